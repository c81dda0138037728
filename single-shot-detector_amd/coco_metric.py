"""COCO bounding-box AP / AR without pycocotools -- the metric of the reference's README.md:3-10 (AP 31.7, AP@0.5 49.8 on val2017).

The reference computes it in inference/evaluate_on_COCO.ipynb cell 17 with `COCOeval(cocoGt, cocoDt, iouType='bbox')` from
cocoapi's PythonAPI (pycocotools: third party, appended to sys.path by cell 0, not vendored by the reference, not installed
here).  This module restates that published algorithm (cocoeval.py `evaluate` / `computeIoU` / `evaluateImg` / `accumulate` /
`summarize`, maskApi.c `bbIou`, coco.py `loadRes` for bbox results) so that `coco_eval.evaluate` ends in the same twelve numbers:

  * per (image, category): detections by descending score (stable), at most 100; IoU of xywh boxes, with a CROWD groundtruth
    box the union is the detection's own area;
  * per area range (all / small < 32^2 / medium / large > 96^2): groundtruth outside the range or crowd is "ignore", sorted behind
    the others; for every IoU threshold 0.50:0.05:0.95 each detection, best score first, takes the still-free groundtruth box of
    the highest IoU >= threshold (a crowd box stays free; once a regular match is held an ignore box cannot replace it); a
    detection matched to an ignore box, or unmatched with its own area outside the range, is ignored;
  * per (category, area range, maxDets 1 / 10 / 100): detections of all images merged by descending score (stable), cumulative
    TP / FP over the non-ignored ones, recall = TP / #non-ignored groundtruth, precision made non-increasing from the right and
    sampled at the 101 recall points 0:0.01:1 (0 beyond the reached recall);
  * AP = mean over thresholds, recall points and categories with groundtruth; AP50 / AP75; APs / APm / APl; AR@1 / @10 / @100;
    ARs / ARm / ARl.
Groundtruth `ignore` = `iscrowd` (bbox evaluation).  Known answers and an independently written brute-force AP are in
tests/test_host.py; no pycocotools run is reachable offline to compare with."""
import json

import numpy as np

IOU_THRS = np.linspace(0.5, 0.95, int(np.round((0.95 - 0.5) / 0.05)) + 1, endpoint=True)
REC_THRS = np.linspace(0.0, 1.00, int(np.round((1.00 - 0.0) / 0.01)) + 1, endpoint=True)
MAX_DETS = (1, 10, 100)
AREA_RNG = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))
AREA_LBL = ("all", "small", "medium", "large")
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
THR_L = [min(float(t), 1 - 1e-10) for t in IOU_THRS]        # cocoeval.py evaluateImg: iou = min([t, 1 - 1e-10])


def bbox_iou(dt, gt, iscrowd):
    """IoU matrix [D, G] of xywh boxes (maskApi.c bbIou): 0 unless the overlap has positive width and height; for a crowd
    groundtruth box the denominator is the detection's area."""
    dt = np.asarray(dt, np.float64).reshape(-1, 4)
    gt = np.asarray(gt, np.float64).reshape(-1, 4)
    crowd = np.asarray(iscrowd, bool).reshape(-1)
    w = np.minimum(dt[:, None, 0] + dt[:, None, 2], gt[None, :, 0] + gt[None, :, 2]) - np.maximum(dt[:, None, 0], gt[None, :, 0])
    h = np.minimum(dt[:, None, 1] + dt[:, None, 3], gt[None, :, 1] + gt[None, :, 3]) - np.maximum(dt[:, None, 1], gt[None, :, 1])
    ok = (w > 0) & (h > 0)
    inter = np.where(ok, w * h, 0.0)
    da = (dt[:, 2] * dt[:, 3])[:, None]
    ga = (gt[:, 2] * gt[:, 3])[None, :]
    union = np.where(crowd[None, :], da, da + ga - inter)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, inter / union, 0.0)


class CocoBoxEval:
    """groundtruth: the annotation file's dict (or its path): 'images', 'annotations' (image_id, category_id, bbox xywh, area,
    iscrowd), 'categories'.  results: the list of result dicts of evaluate_on_COCO.ipynb cell 10 (image_id, category_id, bbox,
    score), or the path of its JSON.  img_ids / cat_ids default to all of the annotation file (cell 17 sets exactly those)."""

    def __init__(self, groundtruth, results, img_ids=None, cat_ids=None):
        gt = json.load(open(groundtruth)) if isinstance(groundtruth, str) else groundtruth
        dt = json.load(open(results)) if isinstance(results, str) else results
        self.img_ids = sorted(set(img_ids if img_ids is not None else [im["id"] for im in gt["images"]]))
        self.cat_ids = sorted(set(cat_ids if cat_ids is not None else [c["id"] for c in gt["categories"]]))
        known = set(im["id"] for im in gt["images"])
        imgs, cats = set(self.img_ids), set(self.cat_ids)
        self._gts, self._dts = {}, {}
        for a in gt["annotations"]:
            if a["image_id"] in imgs and a["category_id"] in cats:
                crowd = int(a.get("iscrowd", 0))
                area = float(a["area"]) if "area" in a else float(a["bbox"][2] * a["bbox"][3])
                self._gts.setdefault((a["image_id"], a["category_id"]), []).append((list(a["bbox"]), area, crowd))
        for k, d in enumerate(dt):
            if d["image_id"] not in known:          # coco.loadRes asserts this
                raise ValueError("results[%d] names image_id %r, which the annotation file does not have" % (k, d["image_id"]))
            if d["image_id"] in imgs and d["category_id"] in cats:
                bb = list(d["bbox"])
                self._dts.setdefault((d["image_id"], d["category_id"]), []).append((bb, float(bb[2] * bb[3]), float(d["score"])))
        self._rows = None                  # from_records: the detections as flat rows instead of _dts
        self._retained = None
        self.eval_imgs = None
        self.precision = self.recall = self.stats = None

    @classmethod
    def from_records(cls, groundtruth, records, image_ids, label_to_coco_id, score_threshold, device=None, img_ids=None, cat_ids=None,
                     image_hw=None):
        """The evaluator of a run whose detections are the engine's record blocks (ssd.split_records; Detector.detect_many_records),
        unfiltered: no result dict and no tuple per detection is built.  records: int32 [n, 6T + 1], a torch tensor on the GPU or a
        numpy block; image_ids: the id of every record's image (each once, all of them in the annotation file); image_hw: (height,
        width) of every record's ORIGINAL image, which the boxes are scaled to -- default: 'height' and 'width' of the annotation
        file's 'images'; label_to_coco_id: {detector label:
        category id}, a label it lacks is not evaluated; score_threshold: rows with score > threshold count (float32, strict).
        device: None builds the rows with coco_rows.rows_host and keeps them on the host; a CUDA device index or torch.device builds
        them with ssd_coco_rows_count / ssd_coco_rows_fill (coco_rows.rows_device; include/ssd_hip.h "the COCO rows") and leaves the
        boxes and areas on that GPU, where evaluate(device=, unpack=False) matches them.  The rows are those of the dict route --
        coco_eval.detection_records into the ordinary constructor -- bit for bit, so evaluate(), cells(), merge(), accumulate() and
        summarize() give what they give there.  A record the header calls bad raises ValueError naming the image and the row.
        If the annotation file has a (category, image) cell with more than coco_match.MAX_GT groundtruth boxes, which the matching
        kernel leaves to the host loop, the WHOLE call takes the dict route instead: the records are downloaded, detection_records
        builds the result dicts and the ordinary constructor takes them."""
        from . import coco_match, coco_rows
        gt = json.load(open(groundtruth)) if isinstance(groundtruth, str) else groundtruth
        self = cls(gt, [], img_ids, cat_ids)
        ids = [int(i) for i in image_ids]
        if len(ids) != len(records):
            raise ValueError("%d image ids for %d records" % (len(ids), len(records)))
        sizes = {im["id"]: im for im in gt["images"]}
        for k, i in enumerate(ids):
            if i not in sizes:
                raise ValueError("records[%d] names image_id %r, which the annotation file does not have" % (k, i))
            if image_hw is None and ("height" not in sizes[i] or "width" not in sizes[i]):
                raise ValueError("image %r of the annotation file has no 'height' / 'width': pass image_hw" % i)
        if len(set(ids)) != len(ids):
            raise ValueError("image_ids names an image twice")
        hw = np.array([[sizes[i]["height"], sizes[i]["width"]] for i in ids] if image_hw is None else image_hw, np.int32).reshape(-1, 2)
        if len(hw) != len(ids):
            raise ValueError("%d image sizes for %d records" % (len(hw), len(ids)))
        is_tensor = not isinstance(records, np.ndarray)
        if any(len(g) > coco_match.MAX_GT for g in self._gts.values()):
            from .coco_eval import detection_records
            from .ssd import score_filter, split_records
            host = records.cpu().numpy() if is_tensor else records
            results = []
            for i, (h, w), b, l, s, n in zip(ids, hw.tolist(), *split_records(np.ascontiguousarray(host))):
                results += detection_records(None, np.empty((h, w, 0), np.uint8), i, label_to_coco_id, score_threshold,
                                             detections=score_filter(b, l, s, n, np.float32(score_threshold)))
            return cls(gt, results, img_ids, cat_ids)
        # the records of the evaluated images, ascending by id: column c of the [K, m] tables is image img_ids[img_pos[c]]
        pos = {img: k for k, img in enumerate(self.img_ids)}
        take = [k for k in np.argsort(np.array(ids, np.int64), kind="stable").tolist() if ids[k] in pos]
        if take != list(range(len(ids))):
            if is_tensor:
                import torch
                records = records[torch.tensor(take, dtype=torch.int64, device=records.device)]
            else:
                records = records[take]
        ids, hw = [ids[k] for k in take], hw[take]
        cat_at = {c: k for k, c in enumerate(self.cat_ids)}
        label_to_cat = np.full(max([int(l) for l in label_to_coco_id] + [0]) + 1, -1, np.int32)
        for label, cat in label_to_coco_id.items():
            label_to_cat[int(label)] = cat_at.get(cat, -1)
        K = max(len(self.cat_ids), 1)
        if device is None:
            rows = coco_rows.rows_host(records.cpu().numpy() if is_tensor else records, hw, label_to_cat, K, score_threshold, image_ids=ids)
        else:
            rows = coco_rows.rows_device(records, hw, label_to_cat, K, score_threshold, device, image_ids=ids)
        rows["img_pos"] = np.array([pos[i] for i in ids], np.int64)
        self._rows, self._dts = rows, None
        return self

    def _need_dts(self):
        """from_records keeps flat rows; the host loops read _dts: built here, on their first use, from the rows (already in every
        cell's order and truncated, which the loops' own stable sort and truncation leave as they are)."""
        if self._dts is not None:
            return
        r = self._rows
        to_host = lambda x: x if isinstance(x, np.ndarray) else x.cpu().numpy()
        box, area, score = to_host(r["det_box"]).tolist(), to_host(r["det_area"]).tolist(), r["det_score"].tolist()
        flat = r["counts"].reshape(-1).astype(np.int64)
        first = np.cumsum(flat) - flat
        m = max(r["counts"].shape[1], 1)
        self._dts = {}
        for c in np.nonzero(flat)[0].tolist():
            a, b = int(first[c]), int(first[c] + flat[c])
            self._dts[(self.img_ids[int(r["img_pos"][c % m])], self.cat_ids[c // m])] = list(zip(box[a:b], area[a:b], score[a:b]))

    def _rows_pack(self, subset):
        """coco_match.pack()'s dict for the images `subset` from the flat rows of from_records: the groundtruth side by pack() itself
        (the detections' dict empty), the cells that hold detections from the counts, merged in the cell order; det_box / det_area
        stay torch tensors when the rows were built on a GPU."""
        from . import coco_match
        from .coco_accumulate import _ranges
        r = self._rows
        if r.get("gt_of") != tuple(subset):
            r["gt_of"], r["gt"] = tuple(subset), coco_match.pack(self._gts, {}, self.cat_ids, subset)
        g = r["gt"]
        N = max(len(self.img_ids), 1)
        img_arr, cat_arr = np.array(self.img_ids, np.int64), np.array(self.cat_ids, np.int64)
        gkeys = np.array(g["keys"], np.int64).reshape(-1, 2)
        gt_cell = np.searchsorted(cat_arr, gkeys[:, 0]) * N + np.searchsorted(img_arr, gkeys[:, 1])
        counts = r["counts"].astype(np.int64)
        flat = counts.reshape(-1)
        first = np.cumsum(flat) - flat
        col_in = np.isin(r["img_pos"], np.searchsorted(img_arr, np.array(list(subset), np.int64)))
        mask = ((counts > 0) & col_in[None, :]).reshape(-1)
        at = np.nonzero(mask)[0]
        m = max(counts.shape[1], 1)
        det_cell = (at // m) * N + r["img_pos"][at % m]
        det_box, det_area, det_score = r["det_box"], r["det_area"], r["det_score"]
        if not col_in.all():                # rows of images outside the subset lie between the others: gather
            rows = _ranges(first[at], flat[at])
            det_score = det_score[rows]
            if isinstance(det_box, np.ndarray):
                det_box, det_area = det_box[rows], det_area[rows]
            else:
                import torch
                idx = torch.from_numpy(rows).to(det_box.device)
                det_box, det_area = det_box[idx], det_area[idx]
        union = np.union1d(gt_cell, det_cell)
        cells = np.zeros(len(union), coco_match.CELL_DTYPE)
        cells["D"][np.searchsorted(union, det_cell)] = flat[at]
        cells["G"][np.searchsorted(union, gt_cell)] = g["cells"]["G"]
        D, G = cells["D"].astype(np.int64), cells["G"].astype(np.int64)
        cells["det_begin"], cells["gt_begin"] = np.cumsum(D) - D, np.cumsum(G) - G
        keys = list(zip(cat_arr[union // N].tolist(), img_arr[union % N].tolist()))
        return {"keys": keys, "packed": np.ones(len(keys), bool), "cells": cells, "det_box": det_box, "det_area": det_area,
                "det_score": det_score, "gt_box": g["gt_box"], "gt_area": g["gt_area"], "gt_crowd": g["gt_crowd"]}

    def __getattr__(self, name):
        """eval_imgs is a plain attribute: {(category, area index, image): (scores, matched, ignored, gt_ignore)}.  Only after
        evaluate(device, unpack=False) is it absent -- the cells then exist as the packed arrays on the host and the matching's
        outputs on the GPU -- and its first read, which lands here, builds it."""
        if name == "eval_imgs" and self.__dict__.get("_retained") is not None:
            self._unpack_retained()
            return self.__dict__["eval_imgs"]
        raise AttributeError(name)

    # -- cocoeval.py evaluate(): computeIoU + evaluateImg for every (category, area range, image)
    def evaluate(self, img_ids=None, device=None, unpack=True):
        """img_ids: evaluate only these images (a subset of self.img_ids, e.g. one rank's share); the cells of the others come
        from `merge`.  accumulate() / summarize() always run over all self.img_ids.
        device: None runs the host loop; a CUDA device index or torch.device runs the matching of all cells as one launch of
        ssd_coco_match (coco_match.py; include/ssd_hip.h "the COCO box matching") on that GPU's current stream -- the same
        eval_imgs, key for key and bit for bit.  A cell with more groundtruth boxes than the kernel takes is computed by the
        host loop in its place.
        unpack (with a device): False keeps the packed arrays on the host and the matching's outputs on the GPU, where
        accumulate(device=) reads them, and builds no eval_imgs; cells(), merge(), accumulate() or a read of eval_imgs builds
        it on demand, equal to what unpack=True gives."""
        self._retained = None
        self.eval_imgs = {}
        if img_ids is None:
            subset = self.img_ids
        else:
            want = set(img_ids)
            if not want <= set(self.img_ids):
                raise ValueError("img_ids must be a subset of the evaluated image ids")
            subset = [i for i in self.img_ids if i in want]
        if device is not None:
            return self._evaluate_on_gpu(subset, device, unpack=unpack)
        if self._rows is not None:
            self._need_dts()
        for cat in self.cat_ids:
            for img in subset:
                gts = self._gts.get((img, cat), [])
                dts = self._dts.get((img, cat), [])
                if not gts and not dts:
                    continue
                for ai, cell in enumerate(self._evaluate_cell(gts, dts)):
                    self.eval_imgs[(cat, ai, img)] = cell
        return self

    @staticmethod
    def _evaluate_cell(gts, dts):
        """One (category, image) cell -> its (scores, matched, ignored, gt_ignore) per area range."""
        T = len(IOU_THRS)
        maxdet = MAX_DETS[-1]
        out = []
        scores = np.array([d[2] for d in dts], np.float64)
        order = np.argsort(-scores, kind="mergesort")[:maxdet]
        dbox = [dts[i][0] for i in order]
        darea = np.array([dts[i][1] for i in order], np.float64)
        dscore = scores[order]
        gcrowd = np.array([g[2] for g in gts], np.int64)
        garea = np.array([g[1] for g in gts], np.float64)
        ious_all = bbox_iou(dbox, [g[0] for g in gts], gcrowd) if gts and dts else np.zeros((len(dbox), len(gts)))
        for ai, (lo, hi) in enumerate(AREA_RNG):
            if not gts:            # (most cells of a real run: detections of a category the image does not have)
                oor = (darea < lo) | (darea > hi)
                out.append((dscore, np.zeros((T, len(dbox)), bool), np.broadcast_to(oor, (T, len(dbox))), np.zeros(0, bool)))
                continue
            gig = (gcrowd != 0) | (garea < lo) | (garea > hi)
            gind = np.argsort(gig.astype(np.int64), kind="mergesort")
            gig_s, crowd_s = gig[gind], gcrowd[gind]
            ious = ious_all[:, gind]
            D, G = len(dbox), len(gts)
            dtm = np.zeros((T, D), bool)
            dtig = np.zeros((T, D), bool)
            if G and D:
                # (plain Python lists inside the loops: indexing numpy scalars costs more than the comparisons)
                iou_l, ig_l, cr_l = ious.tolist(), gig_s.tolist(), [bool(c) for c in crowd_s.tolist()]
                for ti, t in enumerate(THR_L):
                    gtm = [False] * G
                    row_m, row_ig = dtm[ti], dtig[ti]
                    for di in range(D):
                        best = t
                        m = -1
                        row = iou_l[di]
                        for gi in range(G):
                            if gtm[gi] and not cr_l[gi]:
                                continue                       # already matched, and not a crowd
                            if m > -1 and not ig_l[m] and ig_l[gi]:
                                break                          # a regular match is held: ignore boxes (sorted last) cannot take it
                            if row[gi] < best:
                                continue
                            best = row[gi]
                            m = gi
                        if m == -1:
                            continue
                        row_ig[di] = ig_l[m]
                        row_m[di] = True
                        gtm[m] = True
            out_of_range = (darea < lo) | (darea > hi)
            dtig = dtig | (~dtm & out_of_range[None, :])
            out.append((dscore, dtm, dtig, gig_s))
        return out

    def _evaluate_on_gpu(self, subset, device, timings=None, unpack=True):
        """evaluate()'s cells of `subset` through coco_match: pack, one launch, unpack; eval_imgs in the host loop's order.
        unpack=False: pack and one launch; the outputs stay on the GPU (self._retained)."""
        import time
        from . import coco_match
        self._retained = None
        t0 = time.perf_counter()
        p = self._rows_pack(subset) if self._rows is not None else coco_match.pack(self._gts, self._dts, self.cat_ids, subset)
        t1 = time.perf_counter()
        if not unpack:
            matched, ignored, gt_ignore, _ = coco_match.match_device(p, THR_L, AREA_RNG, device, timings=timings)
            self._retained = {"p": p, "matched": matched, "ignored": ignored, "gt_ignore": gt_ignore,
                              "whole": bool(p["packed"].all()) and list(subset) == list(self.img_ids)}
            del self.eval_imgs             # (__getattr__ builds it on the first read)
            if timings is not None:
                timings.update(pack=t1 - t0)
            return self
        matched, ignored, gt_ignore = coco_match.match(p, THR_L, AREA_RNG, device, timings=timings)
        t2 = time.perf_counter()
        self._unpack(p, matched, ignored, gt_ignore)
        if timings is not None:
            timings.update(pack=t1 - t0, unpack=time.perf_counter() - t2)
        return self

    def _unpack_retained(self):
        """eval_imgs from what evaluate(device, unpack=False) kept: the download and the unpacking it skipped"""
        from . import coco_match
        r = self._retained
        m, i, g = coco_match.download_words(r["matched"], r["ignored"], r["gt_ignore"])
        self.eval_imgs = r["built"] = {}       # (accumulate(device) trusts the GPU's arrays only while eval_imgs is this very dict)
        self._unpack(r["p"], coco_match.unpack_bits(m, len(THR_L)), coco_match.unpack_bits(i, len(THR_L)), g.astype(bool))

    def _unpack(self, p, matched, ignored, gt_ignore):
        """pack()'s dict and the matching's outputs (bool [A, T, nd], [A, T, nd], [A, ng]) -> eval_imgs, the host loop's tuples in its order"""
        cells, score = p["cells"], p["det_score"]
        d0, dn, g0, gn = cells["det_begin"].tolist(), cells["D"].tolist(), cells["gt_begin"].tolist(), cells["G"].tolist()
        out = self.eval_imgs
        n = 0
        for (cat, img), packed in zip(p["keys"], p["packed"].tolist()):
            if not packed:             # more groundtruth boxes than the kernel takes: the host loop, in its place
                for ai, cell in enumerate(self._evaluate_cell(self._gts.get((img, cat), []), self._dts.get((img, cat), []))):
                    out[(cat, ai, img)] = cell
                continue
            a, b, c, d = d0[n], d0[n] + dn[n], g0[n], g0[n] + gn[n]
            n += 1
            s = score[a:b]
            for ai in range(len(AREA_RNG)):
                out[(cat, ai, img)] = (s, matched[ai, :, a:b], ignored[ai, :, a:b], gt_ignore[ai, c:d])

    # -- the cells of evaluate() as a few flat arrays (a subset's evaluation travels between processes this way)
    def cells(self):
        """self.eval_imgs as numpy arrays: keys [n,3] int64 (category, area index, image), D / G [n] (detections, groundtruth
        boxes per cell), scores [sum D] float64, matched / ignored [T, sum D] bool, gt_ignore [sum G] bool."""
        T = len(IOU_THRS)
        items = list(self.eval_imgs.items()) if self.eval_imgs else []
        keys = np.array([k for k, _ in items], np.int64).reshape(-1, 3)
        D = np.array([len(v[0]) for _, v in items], np.int64)
        G = np.array([len(v[3]) for _, v in items], np.int64)
        cat = (lambda xs, empty: np.concatenate(xs, axis=-1) if xs else empty)
        return {"keys": keys, "D": D, "G": G,
                "scores": cat([np.asarray(v[0], np.float64) for _, v in items], np.zeros(0, np.float64)),
                "matched": cat([np.asarray(v[1], bool) for _, v in items], np.zeros((T, 0), bool)),
                "ignored": cat([np.asarray(v[2], bool) for _, v in items], np.zeros((T, 0), bool)),
                "gt_ignore": cat([np.asarray(v[3], bool) for _, v in items], np.zeros(0, bool))}

    def merge(self, cells):
        """Adds the cells another subset's evaluate() produced (the dict of `cells()`); the subsets must be disjoint."""
        if self.eval_imgs is None:
            self.eval_imgs = {}
        self._retained = None              # what a GPU holds no longer is all of eval_imgs
        d0 = np.concatenate([[0], np.cumsum(cells["D"])])
        g0 = np.concatenate([[0], np.cumsum(cells["G"])])
        for n, key in enumerate(cells["keys"].tolist()):
            key = tuple(key)
            if key in self.eval_imgs:
                raise ValueError("cell %r evaluated twice" % (key,))
            a, b = int(d0[n]), int(d0[n + 1])
            self.eval_imgs[key] = (cells["scores"][a:b], cells["matched"][:, a:b], cells["ignored"][:, a:b],
                                   cells["gt_ignore"][int(g0[n]):int(g0[n + 1])])
        self.precision = self.recall = self.stats = None
        return self

    # -- cocoeval.py accumulate()
    def accumulate(self, device=None):
        """device: None runs the host loops below; a CUDA device index or torch.device computes the same precision and recall
        arrays, bit for bit, as one launch of ssd_coco_accumulate (coco_accumulate.py; include/ssd_hip.h "the COCO accumulation")
        on that GPU's current stream.  It reads the matching's outputs where evaluate(device, unpack=False) left them if that call
        covered every image on this GPU without a host-fallback cell (the two calls are ordered by that GPU's current stream: make
        them under the same one); any other eval_imgs -- the host loop's, merged subsets, a fallback cell -- is flattened on the
        host and uploaded."""
        if device is not None:
            return self._accumulate_on_gpu(device)
        if self.eval_imgs is None:
            self.evaluate()
        T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(self.cat_ids), len(AREA_RNG), len(MAX_DETS)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        eps = np.spacing(1)
        for k, cat in enumerate(self.cat_ids):
            for a in range(A):
                E = [self.eval_imgs[(cat, a, img)] for img in self.img_ids if (cat, a, img) in self.eval_imgs]
                if not E:
                    continue
                gig = np.concatenate([e[3] for e in E])
                npig = int(np.count_nonzero(~gig))
                if npig == 0:
                    continue
                for m, maxdet in enumerate(MAX_DETS):
                    sc = np.concatenate([e[0][:maxdet] for e in E])
                    inds = np.argsort(-sc, kind="mergesort")
                    dtm = np.concatenate([e[1][:, :maxdet] for e in E], axis=1)[:, inds]
                    dig = np.concatenate([e[2][:, :maxdet] for e in E], axis=1)[:, inds]
                    tp_sum = np.cumsum(dtm & ~dig, axis=1).astype(np.float64)
                    fp_sum = np.cumsum(~dtm & ~dig, axis=1).astype(np.float64)
                    for t in range(T):
                        tp, fp = tp_sum[t], fp_sum[t]
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + eps)
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr = np.maximum.accumulate(pr[::-1])[::-1] if nd else pr      # non-increasing from the right
                        q = np.zeros(R)
                        pos = np.searchsorted(rc, REC_THRS, side="left")
                        ok = pos < nd
                        q[ok] = pr[pos[ok]]
                        precision[t, :, k, a, m] = q
        self.precision, self.recall = precision, recall
        return self

    def _accumulate_on_gpu(self, device, timings=None):
        """accumulate() through coco_accumulate: the global order by one lexsort, one launch, the two arrays read back.
        timings: a dict that receives 'route' ('retained' | 'upload'), 'pack_order' and accumulate()'s parts in seconds."""
        import time
        from . import coco_accumulate as ca
        from .metric_calls import device_of
        T, A = len(IOU_THRS), len(AREA_RNG)
        t0 = time.perf_counter()
        r = self._retained
        if r is not None and self.__dict__.get("eval_imgs", r.get("built")) is not r.get("built"):
            r = self._retained = None          # the caller replaced eval_imgs: what the GPU holds is not it
        if r is not None and r["whole"] and r["matched"].device == device_of(device):
            q = ca.pack_order(r["p"], self.cat_ids)
            matched, ignored, gt_ignore = r["matched"], r["ignored"], r["gt_ignore"]
        else:
            if self.eval_imgs is None:
                self.evaluate()
            q = ca.pack_cells(self.cells(), self.cat_ids, self.img_ids, A)
            matched, ignored, gt_ignore = q["matched"], q["ignored"], q["gt_ignore"]
        t1 = time.perf_counter()
        self.precision, self.recall = ca.accumulate(q, matched, ignored, gt_ignore, T, A, MAX_DETS, REC_THRS, device, timings=timings)
        if timings is not None:
            timings.update(route="retained" if matched is not q.get("matched") else "upload", pack_order=t1 - t0)
        return self

    # -- cocoeval.py summarize()
    def summarize(self, out=None):
        if self.precision is None:
            self.accumulate()

        def stat(ap, iou=None, area="all", maxdet=100):
            a, m = AREA_LBL.index(area), MAX_DETS.index(maxdet)
            s = self.precision[:, :, :, a, m] if ap else self.recall[:, :, a, m]
            if iou is not None:
                s = s[np.where(np.isclose(IOU_THRS, iou))[0]]
            s = s[s > -1]
            return float(np.mean(s)) if s.size else -1.0
        self.stats = np.array([stat(1), stat(1, 0.5), stat(1, 0.75), stat(1, area="small"), stat(1, area="medium"), stat(1, area="large"),
                               stat(0, maxdet=1), stat(0, maxdet=10), stat(0), stat(0, area="small"), stat(0, area="medium"),
                               stat(0, area="large")])
        if out is not None:
            rows = [("Average Precision", "0.50:0.95", "all", 100), ("Average Precision", "0.50", "all", 100), ("Average Precision", "0.75", "all", 100),
                    ("Average Precision", "0.50:0.95", "small", 100), ("Average Precision", "0.50:0.95", "medium", 100),
                    ("Average Precision", "0.50:0.95", "large", 100), ("Average Recall", "0.50:0.95", "all", 1), ("Average Recall", "0.50:0.95", "all", 10),
                    ("Average Recall", "0.50:0.95", "all", 100), ("Average Recall", "0.50:0.95", "small", 100),
                    ("Average Recall", "0.50:0.95", "medium", 100), ("Average Recall", "0.50:0.95", "large", 100)]
            for (title, iou, area, md), v in zip(rows, self.stats):
                out.write(" %-18s (%s) @[ IoU=%-9s | area=%6s | maxDets=%3d ] = %0.3f\n" % (title, "AP" if "Precision" in title else "AR", iou, area, md, v))
        return self.stats


def evaluate_boxes(groundtruth, results, img_ids=None, cat_ids=None, out=None):
    """The twelve COCO statistics (STAT_NAMES order) of `results` against `groundtruth`."""
    return CocoBoxEval(groundtruth, results, img_ids, cat_ids).evaluate().accumulate().summarize(out)
