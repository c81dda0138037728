"""python -m ssd_amd.prepare_coco --instances instances_train2017.json --output train_annotations/ --labels coco_labels.txt

The "Convert" cells of the reference's data/prepare_COCO.ipynb without pycocotools: one <stem>.json per image of a COCO
instances file, in the form data/create_tfrecords.py (and `python -m ssd_amd.create_tfrecords`) reads, and the label file.

What pycocotools did there, restated: images and categories are taken in file order (a repeated image id keeps its first place and
its last entry); an image's annotations are those with its image_id, in file order, whose `iscrowd` equals 0.  What the notebook
does with a box is kept as it is written, the order of the arguments of min and max included -- on a tie Python returns the
FIRST argument, and an int 0 and a float 0.0 print differently in JSON: the corners are ordered, clamped to the image, and a box
under 1 px in either extent is dropped.  The JSON is json.dump's default text with the notebook's key order.  The output
directory is replaced, as the notebook replaces it; the labels file is written only when it is absent."""
import argparse
import json
import os
import shutil


def image_annotation(image, annotations, names):
    """One image's dict: `image` an entry of "images", `annotations` its entries of "annotations" in file order, `names`
    {category id: name}."""
    height, width = image["height"], image["width"]
    objects = []
    for a in annotations:
        if not a["iscrowd"] == 0:
            continue
        left, top, w, h = a["bbox"]
        right, bottom = left + w, top + h
        # ordered corners: each line sees the one before it
        top = min(top, bottom)
        left = min(left, right)
        bottom = max(top, bottom)
        right = max(left, right)
        # into the image
        top = min(max(0, top), height)
        left = min(max(0, left), width)
        bottom = max(min(height, bottom), 0)
        right = max(min(width, right), 0)
        if bottom - top < 1 or right - left < 1:
            continue
        objects.append({"bndbox": {"ymin": top, "ymax": bottom, "xmax": right, "xmin": left}, "name": names[a["category_id"]]})
    return {"filename": image["file_name"], "size": {"depth": 3, "width": width, "height": height}, "object": objects}


def convert(instances, output, labels):
    """`instances`: the path of an instances JSON (or the loaded dict) -> the number of files written into `output`."""
    source = None
    if not isinstance(instances, dict):
        source = instances
        with open(source) as f:
            instances = json.load(f)
    categories = instances["categories"]
    names = {c["id"]: c["name"] for c in categories}
    images = {}
    for im in instances["images"]:
        images[im["id"]] = im
    per_image = {}
    for a in instances.get("annotations", []):
        per_image.setdefault(a["image_id"], []).append(a)
    for im in images.values():
        if not im["file_name"].endswith(".jpg"):
            raise ValueError("%s: the file name must end in .jpg" % im["file_name"])
    out = os.path.realpath(output)
    for keep in [p for p in (labels, source) if p]:
        if os.path.commonpath([out, os.path.realpath(keep)]) == out:
            raise ValueError("%s: the output directory is replaced and must not hold %s" % (output, keep))
    if labels and not os.path.exists(labels):
        with open(labels, "w") as f:
            for c in categories:
                f.write(c["name"] + "\n")
    shutil.rmtree(output, ignore_errors=True)
    os.mkdir(output)
    for key, im in images.items():
        with open(os.path.join(output, im["file_name"][:-4] + ".json"), "w") as f:
            json.dump(image_annotation(im, per_image.get(key, []), names), f)
    return len(images)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[1])
    p.add_argument("--instances", required=True, help="a COCO instances_*.json")
    p.add_argument("--output", required=True, help="the directory of per-image JSON files (replaced)")
    p.add_argument("--labels", required=True, help="the label file: written when absent, one name per line in category order")
    args = p.parse_args(argv)
    n = convert(args.instances, args.output, args.labels)
    print("number of images:", n)
    print("result is here:", args.output)
    return n


if __name__ == "__main__":
    main()
