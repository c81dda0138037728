"""python -m ssd_amd.prepare_coco and python -m ssd_amd.create_tfrecords (default route: no GPU) against what the reference's
data/prepare_COCO.ipynb and data/create_tfrecords.py define: the JSON text and the labels file exactly; shard names, sizes, the
skip count, the seeded order, the refusals naming the file; every Example read back by tfrecords.parse_example and by
google.protobuf's decoder (equality by PARSE: a map's order on the wire is the writer's choice); a grayscale record's bytes."""
import json
import os
import random
from importlib import import_module

import numpy as np
import pytest

from tests.helpers import data_prep_cases as cases
from tests.helpers import example_protos


@pytest.fixture(scope="module")
def mods(ssd):
    return import_module("ssd_amd.prepare_coco"), import_module("ssd_amd.create_tfrecords"), ssd.tfrecords


# ----------------------------------------------------------------------------- prepare_coco
def test_prepare_coco_writes_the_notebooks_json_and_labels(mods, tmp_path):
    prep = mods[0]
    src, out, labels = tmp_path / "instances.json", tmp_path / "ann", tmp_path / "labels.txt"
    src.write_text(json.dumps(cases.INSTANCES))
    assert prep.main(["--instances", str(src), "--output", str(out), "--labels", str(labels)]) == 2
    assert sorted(os.listdir(out)) == sorted(cases.WANT_JSON)
    for name, text in cases.WANT_JSON.items():
        assert (out / name).read_text() == text, name
    assert labels.read_text() == cases.WANT_LABELS
    # a labels file that is there stays as it is; the directory is replaced
    labels.write_text("mine\n")
    (out / "stale.json").write_text("{}")
    assert prep.convert(cases.INSTANCES, str(out), str(labels)) == 2
    assert labels.read_text() == "mine\n" and sorted(os.listdir(out)) == sorted(cases.WANT_JSON)


def test_prepare_coco_refusals(mods, tmp_path):
    prep = mods[0]
    bad = json.loads(json.dumps(cases.INSTANCES))
    bad["images"][1]["file_name"] = "000004.jpeg"
    with pytest.raises(ValueError, match="000004.jpeg"):
        prep.convert(bad, str(tmp_path / "ann"), str(tmp_path / "labels.txt"))
    assert not (tmp_path / "ann").exists() and not (tmp_path / "labels.txt").exists()
    (tmp_path / "in").mkdir()
    src = tmp_path / "in" / "instances.json"
    src.write_text(json.dumps(cases.INSTANCES))
    with pytest.raises(ValueError, match="replaced"):
        prep.convert(str(src), str(tmp_path / "in"), str(tmp_path / "labels.txt"))
    assert src.exists()


# ----------------------------------------------------------------------------- create_tfrecords
@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("prep")
    return str(root), cases.make_folder(str(root))


def run(mods, root, out, **kw):
    create = mods[1]
    return create.create(os.path.join(root, "images"), os.path.join(root, "annotations"), out, os.path.join(root, "labels.txt"), **kw)


def read_shards(tf, out):
    return {name: list(tf.read_records(os.path.join(out, name))) for name in sorted(os.listdir(out))}


def test_shards_order_skips_and_examples(mods, folder, tmp_path):
    root, entries = folder
    tf = mods[2]
    out = str(tmp_path / "shards")
    os.mkdir(out)
    open(os.path.join(out, "stale.tfrecords"), "w").close()                 # the directory is replaced
    counts = run(mods, root, out, num_shards=3, seed=5)
    assert counts == {"examples": 7, "written": 5, "skipped": 2, "shards": 2, "shard_size": 3}
    shards = read_shards(tf, out)
    assert list(shards) == ["shard-0000.tfrecords", "shard-0001.tfrecords"] and [len(v) for v in shards.values()] == [3, 2]
    # the seeded order: the sorted listing shuffled by random.Random(5), the skipped images left out
    order = sorted(s + ".json" for s in entries)
    random.Random(5).shuffle(order)
    stems = [n[:-5] for n in order if entries[n[:-5]]["kind"] in ("rgb", "gray")]
    records = [r for v in shards.values() for r in v]
    official = example_protos.build()["Example"]
    for stem, record in zip(stems, records):
        e = entries[stem]
        w, h = e["size"]
        want = {"image": [cases.stored_image(e)],
                "ymin": [np.float32(a / h) for a, _b, _c, _d, _n in e["objects"]], "xmin": [np.float32(b / w) for _a, b, _c, _d, _n in e["objects"]],
                "ymax": [np.float32(c / h) for _a, _b, c, _d, _n in e["objects"]], "xmax": [np.float32(d / w) for _a, _b, _c, d, _n in e["objects"]],
                "labels": [cases.LABELS[n] for _a, _b, _c, _d, n in e["objects"]]}
        mine = tf.parse_example(record)
        assert list(mine) == ["image", "xmin", "xmax", "ymin", "ymax", "labels"], stem
        msg = official()
        msg.ParseFromString(record)
        theirs = {k: list(getattr(v, v.WhichOneof("kind")).value) for k, v in msg.features.feature.items()}
        for got in (mine, theirs):
            assert set(got) == set(want), stem
            assert got["image"] == want["image"], stem
            assert got["labels"] == want["labels"], stem
            for k in ("ymin", "xmin", "ymax", "xmax"):
                assert [np.float32(x) for x in got[k]] == want[k], (stem, k)
        # the official encoder's bytes of the same message parse to the same thing, and the pipeline's reader takes the record
        assert tf.parse_example(msg.SerializeToString()) == mine
        image, boxes, labels = tf.read_example(record)
        assert image == want["image"][0] and boxes.shape == (len(e["objects"]), 4) and labels.tolist() == want["labels"]
    # a grayscale record holds an RGB JPEG of the same size: PIL's default save
    from PIL import Image
    import io
    gray = [tf.parse_example(r)["image"][0] for s, r in zip(stems, records) if entries[s]["kind"] == "gray"]
    assert len(gray) == 2
    for blob in gray:
        with Image.open(io.BytesIO(blob)) as im:
            assert im.mode == "RGB" and im.format == "JPEG"
    # the same seed gives the same files; another seed another order
    again = str(tmp_path / "again")
    run(mods, root, again, num_shards=3, seed=5)
    assert {n: open(os.path.join(again, n), "rb").read() for n in os.listdir(again)} == \
        {n: open(os.path.join(out, n), "rb").read() for n in os.listdir(out)}
    one = str(tmp_path / "one")
    counts = run(mods, root, one, num_shards=1, seed=6)
    assert counts["shard_size"] == 7 and counts["shards"] == 1 and os.listdir(one) == ["shard-0000.tfrecords"]
    other = sorted(s + ".json" for s in entries)
    random.Random(6).shuffle(other)
    assert other != order
    assert [tf.parse_example(r)["image"][0] for r in tf.read_records(os.path.join(one, "shard-0000.tfrecords"))] == \
        [cases.stored_image(entries[n[:-5]]) for n in other if entries[n[:-5]]["kind"] in ("rgb", "gray")]


def test_the_command_line_and_the_label_encoding(mods, folder, tmp_path, capsys):
    root, _entries = folder
    create = mods[1]
    assert create.read_labels(os.path.join(root, "labels.txt")) == cases.LABELS
    out = str(tmp_path / "cli")
    counts = create.main(["-i", os.path.join(root, "images"), "-a", os.path.join(root, "annotations"), "-o", out,
                          "-l", os.path.join(root, "labels.txt"), "-s", "2", "--seed", "1"])
    assert counts["shard_size"] == 4 and counts["written"] == 5 and counts["shards"] == 2
    assert "number of skipped images: 2" in capsys.readouterr().out
    empty = tmp_path / "empty.txt"
    empty.write_text("\n \n")
    with pytest.raises(ValueError, match="empty.txt"):
        create.read_labels(str(empty))


def test_refusals_name_the_file(mods, folder, tmp_path):
    root, entries = folder
    ann = os.path.join(root, "annotations")
    out = str(tmp_path / "never")

    def with_annotation(stem, change, match):
        path = os.path.join(ann, stem + ".json")
        saved = open(path).read()
        d = json.loads(saved)
        change(d)
        with open(path, "w") as f:
            json.dump(d, f)
        try:
            with pytest.raises(ValueError, match=match) as e:
                run(mods, root, out, num_shards=2, seed=0)
            assert stem + ".json" in str(e.value)
        finally:
            with open(path, "w") as f:
                f.write(saved)

    def box(d):
        return d["object"][0]["bndbox"]
    with_annotation("a_rgb420", lambda d: d["size"].update(width=63), "64 x 48")                          # the size against the file
    with_annotation("c_gray", lambda d: d["size"].update(height=25), "40 x 24")                           # .. of a grayscale file too
    with_annotation("a_rgb420", lambda d: box(d).update(ymin=box(d)["ymax"]), "ymin >= ymax")             # a == c
    with_annotation("b_rgb444", lambda d: box(d).update(xmin=30, xmax=20), "xmin >= xmax")                # inverted
    with_annotation("b_rgb444", lambda d: box(d).update(xmax=38), "outside the image")                    # d > 1
    with_annotation("a_rgb420", lambda d: box(d).update(ymin=-1), "outside the image")                    # a < 0
    with_annotation("a_rgb420", lambda d: d["object"][0].update(name="horse"), "horse")
    with_annotation("a_rgb420", lambda d: d.update(filename="a_rgb420.png"), r"\.jpg or \.jpeg")
    with_annotation("a_rgb420", lambda d: d["size"].update(width=1), "above 1")
    # the output directory: never an input, nor above one
    for bad in (os.path.join(root, "images"), ann, root, os.path.join(root, "images", "..")):
        with pytest.raises(ValueError, match="replaced"):
            run(mods, root, bad, num_shards=1)
    assert len(os.listdir(ann)) == 7 and len(os.listdir(os.path.join(root, "images"))) == 7
    with pytest.raises(ValueError, match="num_shards"):
        run(mods, root, out, num_shards=0)


def test_serialize_example_equals_the_official_encoders_parse(mods):
    tf = mods[2]
    official = example_protos.build()["Example"]
    for boxes, labels in (([], []), ([(0.25, 0.5, 0.75, 1.0)], [3]), ([(0.0, 0.1, 0.2, 0.3), (0.5, 0.5, 1.0, 1.0)], [0, 300])):
        cols = [[b[k] for b in boxes] for k in range(4)]                   # ymin, xmin, ymax, xmax
        mine = tf.serialize_example(b"\xff\xd8jpeg", cols[1], cols[3], cols[0], cols[2], labels)
        msg = official()
        msg.ParseFromString(mine)
        assert sorted(msg.features.feature) == ["image", "labels", "xmax", "xmin", "ymax", "ymin"]
        assert list(msg.features.feature["image"].bytes_list.value) == [b"\xff\xd8jpeg"]
        assert list(msg.features.feature["labels"].int64_list.value) == labels
        assert msg.features.feature["labels"].WhichOneof("kind") == "int64_list" and msg.features.feature["xmin"].WhichOneof("kind") == "float_list"
        for k, name in enumerate(("ymin", "xmin", "ymax", "xmax")):
            assert list(msg.features.feature[name].float_list.value) == [float(np.float32(v)) for v in cols[k]]
        # the official encoder sorts a map's keys when asked to be deterministic: the same entries, another order, the same parse
        assert tf.parse_example(msg.SerializeToString(deterministic=True)) == tf.parse_example(mine)
        image, b, lab = tf.read_example(mine)
        assert b.tolist() == np.asarray(boxes, np.float32).reshape(-1, 4).tolist() and lab.tolist() == labels
