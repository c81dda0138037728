"""The JPEG encoder's host stage (csrc/jpeg_emit.cpp) and the rules it serves (include/ssd_hip.h, block "the JPEG encoder"), without
a GPU: the numpy restatement of the rules reproduces the coefficients of PIL's files, ssd_jpeg_emit fed those coefficients
reproduces the files byte for byte, the quality scaling follows the rule, every refusal comes back with its own status, the plan
lays a batch out, and the stand-alone program of tests/jpeg_emit_check.cpp runs the emitter into exact-size buffers under the
address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

from tests.helpers import jpeg_enc_cases, jpeg_enc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -5


@pytest.fixture(scope="module")
def L(ssd):
    return import_module("ssd_amd._lib")


def emit(lib, coef, h, w, sampling, quality, capacity=None):
    """(status, bytes) of ssd_jpeg_emit into a buffer of `capacity` (default: the bound) between two guard runs."""
    cap = int(lib.ssd_jpeg_emit_bound(h, w, sampling)) if capacity is None else capacity
    buf = np.full(cap + 64, 0xA5, np.uint8)
    size = ctypes.c_int64(-7)
    coef = np.ascontiguousarray(coef, np.int16)
    rc = lib.ssd_jpeg_emit(coef.ctypes.data, h, w, sampling, quality, buf.ctypes.data + 32, cap, ctypes.byref(size))
    assert np.all(buf[:32] == 0xA5) and np.all(buf[32 + cap:] == 0xA5), "a byte outside the capacity was written"
    return rc, bytes(buf[32:32 + size.value]) if rc == OK else b""


def test_restatement_equals_pil_coefficients_on_the_whole_case_list():
    """216 frames, three components each, luma dummy blocks (DC of the block before, AC zero) included."""
    bad, dummies = [], 0
    for (name, arr, quality, sampling, _blob), p in zip(jpeg_enc_cases.cases(), jpeg_enc_cases.parsed()):
        got = jpeg_enc_ref.coefficients(arr, quality, sampling)
        assert np.array_equal(p["quant"], jpeg_enc_ref.quant_tables(quality)[[0, 1, 1]]), name
        if not all(np.array_equal(g, w) for g, w in zip(got, p["coef"])):
            bad.append(name)
        dummies += len(got[0]) - (-(-arr.shape[0] // 8)) * (-(-arr.shape[1] // 8))
    assert not bad, "%d of 216 differ from PIL, the first: %s" % (len(bad), bad[:5])
    assert dummies > 100, "the list must hold dummy blocks"


def test_emit_reproduces_pil_files_from_pil_coefficients(ssd):
    lib = ssd.lib()
    bad = []
    for (name, arr, quality, sampling, blob), p in zip(jpeg_enc_cases.cases(), jpeg_enc_cases.parsed()):
        h, w = arr.shape[:2]
        rc, got = emit(lib, jpeg_enc_cases.pil_flat(p), h, w, jpeg_enc_cases.CODE[sampling], quality)
        assert len(blob) <= lib.ssd_jpeg_emit_bound(h, w, jpeg_enc_cases.CODE[sampling]), name
        if rc != OK or got != blob:
            bad.append(name)
    assert not bad, "%d of 216 files differ from PIL's, the first: %s" % (len(bad), bad[:5])


def test_dummy_blocks_are_never_read(ssd):
    """The device stage stores dummy blocks as zeros; any other value in them gives the same file."""
    lib = ssd.lib()
    for k in (4 * 18 + 2, 8 * 18 + 8, 11 * 18):             # 6x6, 37x53, 9x130 at 4:2:0: dummy blocks right, below and both
        name, arr, quality, sampling, blob = jpeg_enc_cases.cases()[k]
        assert sampling == "420"
        h, w = arr.shape[:2]
        zeros = jpeg_enc_ref.flat(arr, quality, sampling)
        pil = jpeg_enc_cases.pil_flat(jpeg_enc_cases.parsed()[k])
        assert not np.array_equal(zeros, pil), name
        junk = zeros.copy()
        junk[(zeros == 0) & (pil != 0)] = 0x7FFF
        for coef in (zeros, junk):
            assert emit(lib, coef, h, w, 420, quality) == (OK, blob), name


def test_quality_tables_follow_the_rule(ssd):
    lib = ssd.lib()
    for quality in (1, 49, 50, 100):
        scale = 5000 // quality if quality < 50 else 200 - 2 * quality
        want = [[min(max((b * scale + 50) // 100, 1), 255) for b in base] for base in (jpeg_enc_ref.LUMA, jpeg_enc_ref.CHROMA)]
        got = np.zeros(128, np.uint16)
        assert lib.ssd_jpeg_quant_tables(quality, got.ctypes.data) == OK
        assert got.reshape(2, 64).tolist() == want == jpeg_enc_ref.quant_tables(quality).tolist(), quality
    assert jpeg_enc_ref.quant_tables(1).max() == 255 and np.all(jpeg_enc_ref.quant_tables(100) == 1)
    assert jpeg_enc_ref.quant_tables(50)[0].tolist() == jpeg_enc_ref.LUMA
    for quality in (0, 101, -3):
        assert lib.ssd_jpeg_quant_tables(quality, got.ctypes.data) == INVALID
    assert lib.ssd_jpeg_quant_tables(75, None) == INVALID


def test_refusals_by_status(ssd, L):
    lib = ssd.lib()
    name, arr, quality, sampling, blob = jpeg_enc_cases.cases()[8 * 18 + 8]            # 37 x 53, 4:2:0
    h, w = arr.shape[:2]
    coef = jpeg_enc_cases.pil_flat(jpeg_enc_cases.parsed()[8 * 18 + 8])
    assert emit(lib, coef, h, w, 420, quality) == (OK, blob)
    assert emit(lib, coef, h, w, 420, quality, capacity=len(blob)) == (OK, blob), "the exact size is enough"
    for capacity in (0, 1, 300, 622, 623, len(blob) - 2, len(blob) - 1):
        assert emit(lib, coef, h, w, 420, quality, capacity=capacity)[0] == INVALID, "capacity %d of %d" % (capacity, len(blob))
    for bad_sampling in (422, 440, 411, 0, 1):
        assert emit(lib, coef, h, w, bad_sampling, quality, capacity=1 << 16)[0] == UNSUPPORTED
        assert lib.ssd_jpeg_emit_bound(h, w, bad_sampling) == UNSUPPORTED
    for bh, bw in ((0, w), (h, 0), (-1, w), (h, 65536), (65536, w)):
        assert emit(lib, coef, bh, bw, 420, quality, capacity=1 << 16)[0] == INVALID
        assert lib.ssd_jpeg_emit_bound(bh, bw, 420) == INVALID
    assert lib.ssd_jpeg_emit_bound(65535, 65535, 420) == 1024 + 416 * 6 * 4096 * 4096
    for q in (0, 101):
        assert emit(lib, coef, h, w, 420, q)[0] == INVALID
    out, size = np.zeros(1 << 16, np.uint8), ctypes.c_int64()
    assert lib.ssd_jpeg_emit(None, h, w, 420, quality, out.ctypes.data, out.size, ctypes.byref(size)) == INVALID
    assert lib.ssd_jpeg_emit(coef.ctypes.data, h, w, 420, quality, None, out.size, ctypes.byref(size)) == INVALID
    assert lib.ssd_jpeg_emit(coef.ctypes.data, h, w, 420, quality, out.ctypes.data, out.size, None) == INVALID
    assert lib.ssd_jpeg_emit(coef.ctypes.data, h, w, 420, quality, out.ctypes.data, -1, ctypes.byref(size)) == INVALID
    loud = coef.copy()
    loud[0] = 0x7FFF                            # a DC difference past category 11: no code of the table
    assert emit(lib, loud, h, w, 420, quality)[0] == INVALID
    loud = coef.copy()
    loud[5] = -0x4000                           # an AC value past category 10
    assert emit(lib, loud, h, w, 420, quality)[0] == INVALID
    # the plan
    rows = np.asarray([[h, w, 420, 75]], np.int32)
    table, totals = (L.SsdJpegEncodeImage * 1)(), (ctypes.c_int64 * 4)()
    assert lib.ssd_jpeg_encode_plan(rows.ctypes.data, 1, table, totals) == OK
    assert lib.ssd_jpeg_encode_plan(np.asarray([[h, w, 422, 75]], np.int32).ctypes.data, 1, table, totals) == UNSUPPORTED
    assert lib.ssd_jpeg_encode_plan(rows.ctypes.data, -1, table, totals) == INVALID
    assert lib.ssd_jpeg_encode_plan(None, 1, table, totals) == INVALID
    assert lib.ssd_jpeg_encode_plan(rows.ctypes.data, 1, None, totals) == INVALID
    assert lib.ssd_jpeg_encode_plan(rows.ctypes.data, 1, table, None) == INVALID
    for bh, bw, bq in ((0, 5, 75), (5, 0, 75), (65536, 5, 75), (5, 5, 0), (5, 5, 101)):
        assert lib.ssd_jpeg_encode_plan(np.asarray([[bh, bw, 420, bq]], np.int32).ctypes.data, 1, table, totals) == INVALID
    assert lib.ssd_jpeg_encode_plan(None, 0, None, totals) == OK and list(totals) == [0, 0, 0, 0]


def test_header_constants_and_struct_sizes_match_the_binding(L):
    text = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()

    def define(name):
        return int(re.search(r"#define %s \(?(-?\d+)\)?" % name, text).group(1))
    assert define("SSD_JPEG_SAMPLING_420") == L.SSD_JPEG_SAMPLING_420 == 420 and define("SSD_JPEG_SAMPLING_444") == L.SSD_JPEG_SAMPLING_444 == 444
    assert define("SSD_JPEG_ENC_TILE") == L.SSD_JPEG_ENC_TILE == 256
    body = re.search(r"typedef struct ssd_jpeg_encode_image \{\s*/\* (\d+) bytes(.*?)\} ssd_jpeg_encode_image;", text, re.S)
    assert ctypes.sizeof(L.SsdJpegEncodeImage) == int(body.group(1)) == 72
    fields = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body.group(2), flags=re.S))
    assert [f for f in fields if f not in ("int32_t", "int64_t")] == [f[0] for f in L.SsdJpegEncodeImage._fields_]
    for fn in ("ssd_jpeg_quant_tables", "ssd_jpeg_emit_bound", "ssd_jpeg_emit", "ssd_jpeg_encode_plan", "ssd_jpeg_encode_workspace_bytes",
               "ssd_jpeg_encode"):
        assert fn in L.SIGNATURES and re.search(r"\b%s\(" % fn, text)
        declared = re.search(r"^\w+ %s\((.*?)\);" % fn, re.sub(r"/\*.*?\*/", "", text, flags=re.S), re.S | re.M).group(1)
        assert len(L.SIGNATURES[fn][1]) == len(declared.split(",")), fn


def test_plan_lays_a_batch_out(ssd, L):
    lib = ssd.lib()
    hw = np.asarray([[37, 53], [1, 1], [130, 70], [480, 640]], np.int32)
    for samplings in ((420, 420, 420, 420), (444, 444, 444, 444), (444, 420, 444, 420)):
        table, totals = (L.SsdJpegEncodeImage * 4)(), (ctypes.c_int64 * 4)()
        rows = np.asarray([(a, b, s, 30 + k) for k, ((a, b), s) in enumerate(zip(hw, samplings))], np.int32)
        assert lib.ssd_jpeg_encode_plan(rows.ctypes.data, 4, table, totals) == OK
        hv = [1 if s == 444 else 2 for s in samplings]
        mx = [-(-int(w) // (8 * f)) for (_h, w), f in zip(hw, hv)]
        my = [-(-int(hh) // (8 * f)) for (hh, _w), f in zip(hw, hv)]
        nb = [x * y * (f * f + 2) for x, y, f in zip(mx, my, hv)]
        tiles = [-(-8 * x * y // 256) for x, y in zip(mx, my)]
        frames = [(3 * int(a) * int(b) + 15) // 16 * 16 for a, b in hw]
        assert [(t.height, t.width, t.h, t.v, t.mcus_x, t.mcus_y, t.quality, t.reserved) for t in table] == \
            [(int(a), int(b), f, f, x, y, 30 + k, 0) for k, ((a, b), x, y, f) in enumerate(zip(hw, mx, my, hv))]
        sums = lambda xs: [sum(xs[:k]) for k in range(4)]                       # noqa: E731
        assert [t.block_begin for t in table] == sums(nb) and [t.tile_begin for t in table] == sums(tiles)
        assert [t.coef_offset for t in table] == [64 * s for s in sums(nb)] == [t.plane_offset for t in table]
        assert [t.frame_offset for t in table] == sums(frames)
        assert all(t.frame_offset % 16 == 0 and t.plane_offset % 16 == 0 and (2 * t.coef_offset) % 16 == 0 for t in table)
        assert list(totals) == [64 * sum(nb), 64 * sum(nb), sum(frames), sum(nb)]
        assert lib.ssd_jpeg_encode_workspace_bytes(table, 4) == 64 * sum(nb)
        table[2].tile_begin += 1
        assert lib.ssd_jpeg_encode_workspace_bytes(table, 4) == 0


def test_the_entry_point_refuses_before_any_hip_call(ssd, L):
    """No GPU here: every refusal below returns before the first HIP call, so the 'device' pointers are host addresses the call
    never reads."""
    lib = ssd.lib()
    rows = np.asarray([[37, 53, 420, 75], [8, 8, 420, 90]], np.int32)
    table, totals = (L.SsdJpegEncodeImage * 2)(), (ctypes.c_int64 * 4)()
    assert lib.ssd_jpeg_encode_plan(rows.ctypes.data, 2, table, totals) == OK
    buf = np.zeros(4096, np.uint8)
    fake = buf.ctypes.data + (-buf.ctypes.data) % 16
    names = ("images_dev", "frames_dev", "workspace_dev", "coef_dev")

    def call(B=2, **kw):
        a = dict({n: fake for n in names}, **kw)
        rc = lib.ssd_jpeg_encode(table, a["images_dev"], B, a["frames_dev"], a["workspace_dev"], a["coef_dev"], None)
        return rc, lib.ssd_last_error().decode()

    def refused(word, status=INVALID, **kw):
        rc, msg = call(**kw)
        assert rc == status and msg == "ssd_jpeg_encode: " + word, (rc, msg)

    for name, align in zip(names, (8, 1, 16, 16)):
        refused(name + " is NULL", **{name: None})
        if align > 1:
            refused("%s must be %d-byte aligned" % (name, align), **{name: fake + align // 2})
    refused("B must be in [0, 2^20]", B=-1)
    assert call(B=0, **{n: None for n in names})[0] == OK
    assert lib.ssd_jpeg_encode(None, None, 0, None, None, None, None) == OK

    def with_row(word, status=INVALID, **fields):
        saved = {k: getattr(table[1], k) for k in fields}
        for k, v in fields.items():
            setattr(table[1], k, v)
        try:
            refused("images_host[1]" + word, status)
        finally:
            for k, v in saved.items():
                setattr(table[1], k, v)
    with_row(": the sampling must be 4:4:4 (1x1) or 4:2:0 (2x2)", UNSUPPORTED, v=1)                    # 4:2:2
    with_row(": height and width must be in [1, 65535], mcus_x and mcus_y their MCU counts", height=0)
    with_row(": height and width must be in [1, 65535], mcus_x and mcus_y their MCU counts", mcus_x=2)
    with_row(".quality must be in [1, 100]", quality=0)
    with_row(".quality must be in [1, 100]", quality=101)
    with_row(".frame_offset must be in [0, 2^40]", frame_offset=-1)
    with_row(".plane_offset must be a multiple of 16 behind the planes before it", plane_offset=table[1].plane_offset + 8)
    with_row(".plane_offset must be a multiple of 16 behind the planes before it", plane_offset=table[1].plane_offset - 16)
    with_row(".coef_offset must be a multiple of 8 behind the coefficients before it", coef_offset=table[1].coef_offset + 4)
    with_row(".coef_offset must be a multiple of 8 behind the coefficients before it", coef_offset=table[1].coef_offset - 8)
    with_row(".block_begin must be the blocks of the images before", block_begin=table[1].block_begin + 1)
    with_row(".tile_begin must be the tiles of the images before", tile_begin=0)


# ----------------------------------------------------------------------------- the emitter under the sanitizers
def test_emitter_under_sanitizers_into_exact_size_buffers(tmp_path):
    """tests/jpeg_emit_check.cpp + csrc/jpeg_emit.cpp alone, built with -fsanitize=address,undefined: the 216 cases with the
    coefficients and the output in exact-size heap buffers, and every capacity from 0 to the bound - 1 for three of them."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_emit_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "jpeg_emit_check.cpp"), os.path.join(ROOT, "single-shot-detector_amd", "csrc", "jpeg_emit.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and re.search(r"asan|ubsan|sanitize", built.stderr):
        pytest.skip("the sanitizer runtime is absent: %s" % built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr
    corpus = str(tmp_path / "corpus.bin")
    jpeg_enc_cases.write_corpus(corpus, sweep=3)
    run = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    cases, sweeps, capacities = [int(v) for v in re.search(r"cases (\d+) sweeps (\d+) capacities (\d+)", run.stdout).groups()]
    assert cases == 216 and sweeps == 3 and capacities > 3 * 1024
