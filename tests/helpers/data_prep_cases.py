"""The data-preparation tests' inputs, made at test time: a hand-written COCO instances dict for prepare_coco, and a folder of
seven images with their annotation files for create_tfrecords (host and GPU tests share it)."""
import io
import json
import os

import numpy as np

from tests.helpers import jpeg_cases

# categories with non-contiguous ids, in a file order that is not the id order
INSTANCES = {
    "images": [{"id": 9, "file_name": "000009.jpg", "height": 100, "width": 200},
               {"id": 4, "file_name": "000004.jpg", "height": 50, "width": 60}],
    "categories": [{"id": 7, "name": "cat"}, {"id": 2, "name": "traffic light"}, {"id": 90, "name": "dog"}],
    "annotations": [
        {"id": 1, "image_id": 9, "category_id": 90, "bbox": [10.5, 20.0, 30.25, 40.0], "iscrowd": 0},
        {"id": 2, "image_id": 9, "category_id": 7, "bbox": [0, 0, 50, 50], "iscrowd": 1},                 # a crowd box: left out
        {"id": 3, "image_id": 9, "category_id": 2, "bbox": [150.0, 80.0, 100.0, 40.0], "iscrowd": 0},     # past the right and bottom border
        {"id": 4, "image_id": 9, "category_id": 7, "bbox": [5.0, 5.0, 0.5, 30.0], "iscrowd": 0},          # under 1 px wide: dropped
        {"id": 5, "image_id": 9, "category_id": 7, "bbox": [-3.0, 0.0, 20.0, 10.0], "iscrowd": 0},        # past the left border, top on it
    ]}
# json.dump's default text of what the notebook builds: its key order; max(0, -3.0) is the int 0, min(max(0, 0.0), h) the int 0
WANT_JSON = {
    "000009.json": '{"filename": "000009.jpg", "size": {"depth": 3, "width": 200, "height": 100}, "object": ['
                   '{"bndbox": {"ymin": 20.0, "ymax": 60.0, "xmax": 40.75, "xmin": 10.5}, "name": "dog"}, '
                   '{"bndbox": {"ymin": 80.0, "ymax": 100, "xmax": 200, "xmin": 150.0}, "name": "traffic light"}, '
                   '{"bndbox": {"ymin": 0, "ymax": 10.0, "xmax": 17.0, "xmin": 0}, "name": "cat"}]}',
    "000004.json": '{"filename": "000004.jpg", "size": {"depth": 3, "width": 60, "height": 50}, "object": []}',
}
WANT_LABELS = "cat\ntraffic light\ndog\n"

LABELS_TEXT = "cat\n\ndog\n  bird \n"         # a blank line counts: cat 0, dog 2, bird 3
LABELS = {"cat": 0, "dog": 2, "bird": 3}


def _save(arr, path, **kw):
    from PIL import Image
    Image.fromarray(arr).save(path, **kw)


def make_folder(root):
    """images/, annotations/ and labels.txt under `root`: seven annotation files -- 4:2:0 and 4:4:4 RGB JPEGs, two grayscale JPEGs
    (one with a height and width that leave dummy blocks), a second 4:2:0 RGB, a CMYK JPEG and a PNG under a .jpg name (both
    skipped).  -> {stem: dict(kind, size (w, h), objects [(ymin, xmin, ymax, xmax, name)])}."""
    from PIL import Image
    images, anns = os.path.join(root, "images"), os.path.join(root, "annotations")
    os.mkdir(images), os.mkdir(anns)
    with open(os.path.join(root, "labels.txt"), "w") as f:
        f.write(LABELS_TEXT)
    spec = {
        "a_rgb420": ("rgb", (64, 48), {"format": "JPEG", "quality": 90}),
        "b_rgb444": ("rgb", (37, 53), {"format": "JPEG", "quality": 85, "subsampling": 0}),
        "c_gray": ("gray", (40, 24), {"format": "JPEG", "quality": 92}),
        "d_gray_odd": ("gray", (53, 37), {"format": "JPEG", "quality": 60}),
        "e_cmyk": ("cmyk", (32, 32), {"format": "JPEG"}),
        "f_png": ("png", (20, 30), {"format": "PNG"}),
        "g_rgb420": ("rgb", (33, 65), {"format": "JPEG"}),
    }
    out = {}
    for k, (stem, (kind, (w, h), kw)) in enumerate(spec.items()):
        arr = jpeg_cases.pixels(h, w, "ramp", 40 + k)
        name = stem + (".jpeg" if stem == "b_rgb444" else ".jpg")
        path = os.path.join(images, name)
        if kind == "gray":
            _save(arr[:, :, 0], path, **kw)
        elif kind == "cmyk":
            Image.fromarray(arr).convert("CMYK").save(path, **kw)
        else:
            _save(arr, path, **kw)
        objects = [(1, 2, h - 3, w - 1, "dog"), (0, 0, h, w // 2, "bird")][:1 + k % 2] if stem != "g_rgb420" else []
        with open(os.path.join(anns, stem + ".json"), "w") as f:
            json.dump({"filename": name, "size": {"depth": 3, "width": w, "height": h},
                       "object": [{"bndbox": {"ymin": a, "ymax": c, "xmax": d, "xmin": b}, "name": n} for a, b, c, d, n in objects]}, f)
        out[stem] = {"kind": kind, "size": (w, h), "objects": objects, "path": path}
    return out


def stored_image(entry):
    """The bytes the reference stores for a written image: the file's own, or for a grayscale file PIL's default save of its
    array stacked three times (create_tfrecords.py: to_jpeg_bytes)."""
    from PIL import Image
    with open(entry["path"], "rb") as f:
        blob = f.read()
    if entry["kind"] != "gray":
        return blob
    y = np.array(Image.open(io.BytesIO(blob)))
    buf = io.BytesIO()
    Image.fromarray(np.stack(3 * [y], axis=2)).save(buf, format="jpeg")
    return buf.getvalue()
