"""The COCO box matching's test set (include/ssd_hip.h, "the COCO box matching"): a small random annotation file and result list
plus one crafted image, and an instrumented restatement of CocoBoxEval.evaluate's loops that counts how often every branch of
the scan is taken -- the tests assert each counter positive, so a changed generator cannot quietly stop covering a branch.

Random part, n_img images x n_cat categories: a cell is empty, detections only, groundtruth only, or both.  Groundtruth boxes have
integer corners in [0, 60) and sides from SIDES, so areas land exactly on 32^2 and 96^2; a box is duplicated with probability 0.25
(equal IoUs) and is a crowd with probability 0.2.  1 to 9 detections per cell; 80 % are copies of a groundtruth box with integer
jitter in [-3, 3] (applied with probability 0.7), the others stray squares; scores come from SCORES as float32 values (ties).
Crafted part, image n_img + 1: IoUs of exactly 0.5 and 0.75, a category with 130 detections on one crowd and one regular box, a
category with 70 groundtruth boxes and 40 detections."""
import collections

import numpy as np

SIDES = [6, 16, 31, 32, 33, 64, 95, 96, 97, 150]
SCORES = [0.2, 0.35, 0.35, 0.5, 0.5, 0.5, 0.75, 0.9]
SEEDS = (0, 1, 2)
BRANCHES = ("skip taken", "break: regular match held", "tie: later box wins", "ignore box replaces ignore box",
            "IoU equals the threshold", "crowd box taken again", "matched to ignore", "matched to regular", "unmatched, in range",
            "unmatched, out of range", "groundtruth area on a range bound", "detection area on a range bound",
            "reordered groundtruth", "cells with tied scores", "cells without groundtruth", "cells without detections",
            "cells over 100 detections")


def make(seed, n_img=12, n_cat=6, crafted=True):
    """-> (annotation dict, result list)"""
    rng = np.random.default_rng(seed)
    anns, dets = [], []
    for img in range(1, n_img + 1):
        for cat in range(1, n_cat + 1):
            kind = rng.integers(0, 8)                          # 0: empty cell, 1: detections only, 2: groundtruth only, else both
            if kind == 0:
                continue
            ng = 0 if kind == 1 else int(rng.integers(1, 7))
            gts = []
            for _ in range(ng):
                s, s2 = rng.choice(SIDES, 2)
                x, y = rng.integers(0, 60, 2)
                bb = [int(x), int(y), int(s), int(s2 if rng.random() < 0.5 else s)]
                gts.append(bb)
                if rng.random() < 0.25:
                    gts.append(list(bb))                       # a duplicate box: equal IoUs
            for bb in gts:
                anns.append({"image_id": img, "category_id": cat, "bbox": bb, "area": float(bb[2] * bb[3]), "iscrowd": int(rng.random() < 0.2)})
            if kind == 2:
                continue
            for _ in range(int(rng.integers(1, 10))):
                if gts and rng.random() < 0.8:
                    b = gts[rng.integers(len(gts))]
                    j = rng.integers(-3, 4, 4) * (rng.random() < 0.7)
                    bb = [b[0] + int(j[0]), b[1] + int(j[1]), max(1, b[2] + int(j[2])), max(1, b[3] + int(j[3]))]
                else:
                    s = int(rng.choice(SIDES))
                    bb = [int(rng.integers(0, 60)), int(rng.integers(0, 60)), s, s]
                dets.append({"image_id": img, "category_id": cat, "bbox": bb, "score": float(np.float32(rng.choice(SCORES)))})
    n_images = n_img
    if crafted:
        img = n_images = n_img + 1
        anns += [{"image_id": img, "category_id": 1, "bbox": [0, 0, 10, 20], "area": 200.0, "iscrowd": 0},
                 {"image_id": img, "category_id": 1, "bbox": [100, 0, 40, 10], "area": 400.0, "iscrowd": 0}]
        dets += [{"image_id": img, "category_id": 1, "bbox": [0, 0, 10, 10], "score": 0.9},          # IoU exactly 0.5
                 {"image_id": img, "category_id": 1, "bbox": [100, 0, 30, 10], "score": 0.8}]        # IoU exactly 0.75
        for i in range(130):
            dets.append({"image_id": img, "category_id": 2, "bbox": [i % 13, i % 7, 40, 40], "score": float(np.float32(0.2 + (i % 50) / 100.0))})
        anns.append({"image_id": img, "category_id": 2, "bbox": [3, 3, 40, 40], "area": 1600.0, "iscrowd": 1})
        anns.append({"image_id": img, "category_id": 2, "bbox": [5, 2, 40, 40], "area": 1600.0, "iscrowd": 0})
        for i in range(70):
            anns.append({"image_id": img, "category_id": 3, "bbox": [i, 2 * (i % 9), 30 + i % 5, 30], "area": float((30 + i % 5) * 30),
                         "iscrowd": int(i % 11 == 0)})
        for i in range(40):
            dets.append({"image_id": img, "category_id": 3, "bbox": [i * 2, 2 * (i % 9), 31, 30], "score": float(np.float32(0.3 + (i % 7) / 10.0))})
    gt = {"images": [{"id": i} for i in range(1, n_images + 1)], "annotations": anns, "categories": [{"id": c} for c in range(1, n_cat + 1)]}
    return gt, dets


def branch_counts(ev, cm):
    """The loops of CocoBoxEval.evaluate (cm = the coco_metric module, ev = a CocoBoxEval) with a counter on every branch."""
    cnt = collections.Counter()
    for cat in ev.cat_ids:
        for img in ev.img_ids:
            gts, dts = ev._gts.get((img, cat), []), ev._dts.get((img, cat), [])
            if not gts and not dts:
                continue
            cnt["cells"] += 1
            scores = np.array([d[2] for d in dts], np.float64)
            if len(dts) > 100:
                cnt["cells over 100 detections"] += 1
            if len(set(scores.tolist())) < len(scores):
                cnt["cells with tied scores"] += 1
            order = np.argsort(-scores, kind="mergesort")[:100]
            dbox = [dts[i][0] for i in order]
            darea = np.array([dts[i][1] for i in order], np.float64)
            if not gts:
                cnt["cells without groundtruth"] += 1
                continue
            if not dts:
                cnt["cells without detections"] += 1
                continue
            gcrowd = np.array([g[2] for g in gts], np.int64)
            garea = np.array([g[1] for g in gts], np.float64)
            ious_all = cm.bbox_iou(dbox, [g[0] for g in gts], gcrowd)
            for lo, hi in cm.AREA_RNG:
                gig = (gcrowd != 0) | (garea < lo) | (garea > hi)
                if ((garea == lo) | (garea == hi)).any():
                    cnt["groundtruth area on a range bound"] += 1
                if ((darea == lo) | (darea == hi)).any():
                    cnt["detection area on a range bound"] += 1
                gind = np.argsort(gig.astype(np.int64), kind="mergesort")
                if not np.array_equal(gind, np.arange(len(gts))):
                    cnt["reordered groundtruth"] += 1
                ig, cr, iou = gig[gind].tolist(), [bool(c) for c in gcrowd[gind]], ious_all[:, gind].tolist()
                for t in cm.THR_L:
                    gtm = [False] * len(gts)
                    for di in range(len(dbox)):
                        best, m = t, -1
                        for gi in range(len(gts)):
                            if gtm[gi] and not cr[gi]:
                                cnt["skip taken"] += 1
                                continue
                            if m > -1 and not ig[m] and ig[gi]:
                                cnt["break: regular match held"] += 1
                                break
                            if iou[di][gi] < best:
                                continue
                            if m > -1 and iou[di][gi] == best:
                                cnt["tie: later box wins"] += 1
                            if m > -1 and ig[m] and ig[gi]:
                                cnt["ignore box replaces ignore box"] += 1
                            if iou[di][gi] == t:
                                cnt["IoU equals the threshold"] += 1
                            if gtm[gi] and cr[gi]:
                                cnt["crowd box taken again"] += 1
                            best, m = iou[di][gi], gi
                        if m == -1:
                            cnt["unmatched, out of range" if darea[di] < lo or darea[di] > hi else "unmatched, in range"] += 1
                            continue
                        cnt["matched to ignore" if ig[m] else "matched to regular"] += 1
                        gtm[m] = True
    return cnt
