"""The JPEG decoder's host stage (csrc/jpeg_host.cpp) and the rules it serves (include/ssd_hip.h, block "the JPEG decoder"), without a
GPU: the numpy restatement of the rules reproduces PIL bit for bit, ssd_jpeg_entropy reproduces the restatement's coefficients, every
refusal comes back with its own status, no prefix of a file is accepted, and the stand-alone program of tests/jpeg_host_check.cpp
runs the parser over damaged inputs under the address and undefined-behaviour sanitizers."""
import ctypes
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests.helpers import jpeg_cases, jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -5


@pytest.fixture(scope="module")
def host(ssd):
    """(info_read(blob) -> (rc, info), entropy(blob, info) -> (rc, coef, quant)) on the library's entry points."""
    L = import_lib(ssd)
    lib = ssd.lib()

    def info_read(blob):
        info = L.SsdJpegInfo()
        return lib.ssd_jpeg_info_read(blob, len(blob), ctypes.byref(info)), info

    def entropy(blob, info):
        coef = np.full(int(info.coef_count), 0x5A5A, np.int16)
        quant = np.full(64 * int(info.components), 0xA5A5, np.uint16)
        rc = lib.ssd_jpeg_entropy(blob, len(blob), ctypes.byref(info), coef.ctypes.data, quant.ctypes.data)
        return rc, coef, quant
    return info_read, entropy


def import_lib(ssd):
    from importlib import import_module
    return import_module("ssd_amd._lib")


def status(host, blob):
    """The status a caller sees: ssd_jpeg_info_read's refusal, else ssd_jpeg_entropy's."""
    info_read, entropy = host
    rc, info = info_read(blob)
    return rc if rc != OK else entropy(blob, info)[0]


@pytest.fixture(scope="module")
def parsed():
    """The restatement's parse of every case, once."""
    return [jpeg_ref.parse(blob) for _name, blob in jpeg_cases.cases()]


def test_restatement_equals_pil_on_the_whole_case_list(parsed):
    bad = [name for (name, _b), p, want in zip(jpeg_cases.cases(), parsed, jpeg_cases.expected())
           if not np.array_equal(jpeg_ref.pixels(p), want)]
    assert not bad, "%d of %d differ from PIL, the first: %s" % (len(bad), len(parsed), bad[:5])


def test_every_case_is_pinned_with_room(parsed):
    """None of the 432 files comes near a limb of the header's "pinned streams" rule: a factor 2 below each of them."""
    worst = np.array([jpeg_ref.ranges(p) for p in parsed])
    assert all(jpeg_ref.pinned(p) for p in parsed)
    assert worst[:, 0].max() * 2 <= jpeg_ref.X_LIMIT and worst[:, 1].max() * 2 <= jpeg_ref.W_LIMIT
    assert worst[:, 2].min() * 2 >= jpeg_ref.V_MIN and worst[:, 3].max() * 2 <= jpeg_ref.V_MAX


def test_entropy_stage_equals_the_restatement(host, parsed):
    info_read, entropy = host
    for (name, blob), p in zip(jpeg_cases.cases(), parsed):
        rc, info = info_read(blob)
        assert rc == OK, name
        assert (info.height, info.width, info.components, info.h, info.v, info.mcus_x, info.mcus_y, info.restart_interval) == \
            (p["height"], p["width"], p["components"], p["h"], p["v"], p["mcus_x"], p["mcus_y"], p["restart"]), name
        assert list(info.blocks)[:p["components"]] == [len(c) for c in p["coef"]], name
        rc, coef, quant = entropy(blob, info)
        assert rc == OK, name
        assert np.array_equal(coef, np.concatenate([c.reshape(-1) for c in p["coef"]])), name
        assert np.array_equal(quant, p["quant"].reshape(-1)), name


def test_info_fields_on_known_files(host):
    info_read, _ = host
    arr = jpeg_cases.pixels(37, 53, "ramp", 1)
    want = {"444": (1, 1, 7, 5, 35, 35, 35), "422": (2, 1, 4, 5, 40, 20, 20), "420": (2, 2, 4, 3, 48, 12, 12), "gray": (1, 1, 7, 5, 35, 0, 0)}
    for sampling, (h, v, mx, my, b0, b1, b2) in want.items():
        rc, info = info_read(jpeg_cases.encode(arr, sampling, 90))
        assert rc == OK
        assert (info.height, info.width, info.components) == (37, 53, 1 if sampling == "gray" else 3)
        assert (info.h, info.v, info.mcus_x, info.mcus_y, list(info.blocks)) == (h, v, mx, my, [b0, b1, b2])
        assert info.coef_count == 64 * (b0 + b1 + b2) and info.restart_interval == 0 and info.reserved == 0
    rc, info = info_read(jpeg_cases.encode(arr, "420", 90, restart_marker_blocks=3))
    assert rc == OK and info.restart_interval == 3


# ----------------------------------------------------------------------------- refusals
def _segments(blob):
    """[(marker, start of FF, end)] of the segments in front of the scan data."""
    out, p = [], 2
    while True:
        assert blob[p] == 0xFF
        m, n = blob[p + 1], struct.unpack(">H", blob[p + 2:p + 4])[0]
        out.append((m, p, p + 2 + n))
        p += 2 + n
        if m == 0xDA:
            return out


def _find(blob, marker):
    return next((a, b) for m, a, b in _segments(blob) if m == marker)


def _base(sampling="444", h=16, w=16, quality=90, **kw):
    return jpeg_cases.encode(jpeg_cases.pixels(h, w, "ramp", 5), sampling, quality, **kw)


def test_refusals_by_reason(host):
    from PIL import Image
    arr = jpeg_cases.pixels(16, 16, "ramp", 5)
    base = _base()
    assert status(host, base) == OK

    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", progressive=True)
    assert status(host, buf.getvalue()) == UNSUPPORTED, "progressive"
    buf = io.BytesIO()
    Image.fromarray(arr).convert("CMYK").save(buf, "JPEG")
    assert status(host, buf.getvalue()) == UNSUPPORTED, "CMYK: 4 components"

    a, _ = _find(base, 0xC0)
    for factors in (0x12, 0x41):                # luma 1x2 (4:4:0) and 4x1 (4:1:1)
        patched = bytearray(base)
        patched[a + 11] = factors
        assert status(host, bytes(patched)) == UNSUPPORTED, "luma sampling %02x" % factors
    patched = bytearray(base)
    patched[a + 4] = 12                         # the precision byte
    assert status(host, bytes(patched)) == UNSUPPORTED, "12-bit precision"
    patched = bytearray(base)
    patched[a + 5:a + 7] = b"\0\0"              # height 0: DNL
    assert status(host, bytes(patched)) == UNSUPPORTED, "height 0"

    sa, _ = _find(base, 0xDA)
    assert base[-2:] == b"\xff\xd9"
    assert status(host, base[:-2] + base[sa:]) == UNSUPPORTED, "a second scan"

    ja, jb = _find(base, 0xE0)                  # JFIF -> an Adobe segment
    for transform, want in ((0, UNSUPPORTED), (1, OK), (2, UNSUPPORTED)):
        adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])
        assert status(host, base[:ja] + adobe + base[jb:]) == want, "Adobe transform %d" % transform
    plain = base[:ja] + base[jb:]               # neither marker: by the component ids
    assert status(host, plain) == OK
    ca, _ = _find(plain, 0xC0)
    sa2, _ = _find(plain, 0xDA)
    rgb = bytearray(plain)
    for k, ch in enumerate(b"RGB"):
        rgb[ca + 10 + 3 * k] = ch
        rgb[sa2 + 5 + 2 * k] = ch
    assert status(host, bytes(rgb)) == UNSUPPORTED, "component ids R, G, B"

    qa, _ = _find(base, 0xDB)                   # every table value 255: the DC term alone passes 32767
    loud = bytearray(jpeg_cases.encode(np.full((16, 16, 3), 250, np.uint8), "444", 90))
    for m, a2, b2 in _segments(bytes(loud)):
        if m == 0xDB:
            for p in range(a2 + 4, b2, 65):
                loud[p + 1:p + 65] = b"\xff" * 64
    info_read, entropy = host
    rc, info = info_read(bytes(loud))
    assert rc == OK and entropy(bytes(loud), info)[0] == UNSUPPORTED, "|coefficient * q| > 32767"
    patched = bytearray(base)
    patched[qa + 4] = 0x10                      # Pq = 1: a 16-bit table
    assert status(host, bytes(patched)) == UNSUPPORTED, "16-bit quantisation table"

    assert status(host, b"") == INVALID and status(host, b"\x89PNG\r\n\x1a\n" + bytes(32)) == INVALID
    info_read, entropy = host
    rc, info = info_read(base)
    other = _base("420")
    assert entropy(other, info)[0] == INVALID, "an info of other bytes"


def test_no_prefix_is_accepted(host):
    for blob in (_base("420", 9, 11), _base("gray", 16, 8, restart_marker_blocks=1)):
        assert status(host, blob) == OK
        for n in range(len(blob)):
            assert status(host, blob[:n]) in (INVALID, UNSUPPORTED), "the first %d of %d bytes" % (n, len(blob))


def test_header_constants_and_struct_sizes_match_the_binding(ssd):
    L = import_lib(ssd)
    text = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()

    def define(name):
        return int(re.search(r"#define %s \(?(-?\d+)\)?" % name, text).group(1))
    assert define("SSD_ERR_UNSUPPORTED") == L.SSD_ERR_UNSUPPORTED == UNSUPPORTED and define("SSD_ERR_INVALID") == L.SSD_ERR_INVALID
    assert define("SSD_JPEG_RUN") == L.SSD_JPEG_RUN and define("SSD_JPEG_TILE") == L.SSD_JPEG_TILE == 256 * L.SSD_JPEG_RUN
    for cls, name in ((L.SsdJpegInfo, "ssd_jpeg_info"), (L.SsdJpegImage, "ssd_jpeg_image")):
        body = re.search(r"typedef struct %s \{\s*/\* (\d+) bytes(.*?)\} %s;" % (name, name), text, re.S)
        assert ctypes.sizeof(cls) == int(body.group(1))
        fields = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body.group(2), flags=re.S))
        assert [f for f in fields if f not in ("int32_t", "int64_t")] == [f[0] for f in cls._fields_], name
    for fn in ("ssd_jpeg_info_read", "ssd_jpeg_entropy", "ssd_jpeg_plan", "ssd_jpeg_workspace_bytes", "ssd_jpeg_decode"):
        assert fn in L.SIGNATURES and re.search(r"\b%s\(" % fn, text)


def test_plan_lays_a_batch_out(ssd, host):
    L = import_lib(ssd)
    info_read, _ = host
    infos = [info_read(_base(s, h, w))[1] for s, h, w in (("420", 37, 53), ("gray", 1, 1), ("422", 130, 70))]
    arr = (L.SsdJpegInfo * 3)(*infos)
    table, totals = (L.SsdJpegImage * 3)(), (ctypes.c_int64 * 4)()
    assert ssd.lib().ssd_jpeg_plan(arr, 3, table, totals) == OK
    nb = [sum(i.blocks) for i in infos]
    assert [t.block_begin for t in table] == [0, nb[0], nb[0] + nb[1]] and [t.coef_offset for t in table] == [0, 64 * nb[0], 64 * (nb[0] + nb[1])]
    assert [t.tile_begin for t in table] == [0, 1, 2] and [t.quant_offset for t in table] == [0, 192, 256]
    assert [t.frame_offset for t in table] == [0, (37 * 53 * 3 + 15) // 16 * 16, (37 * 53 * 3 + 15) // 16 * 16 + 16]
    assert list(totals) == [64 * sum(nb), 448, 64 * sum(nb), table[2].frame_offset + (130 * 70 * 3 + 15) // 16 * 16]
    arr[1].mcus_x = 2
    assert ssd.lib().ssd_jpeg_plan(arr, 3, table, totals) == INVALID


def test_the_entry_point_refuses_before_any_hip_call(ssd, host):
    """No GPU here: every refusal below returns before the first HIP call, so the 'device' pointers are host addresses the call
    never reads."""
    L, lib = import_lib(ssd), ssd.lib()
    info_read, _ = host
    rc, info = info_read(_base("gray", 1, 1))
    assert rc == OK
    table, totals = (L.SsdJpegImage * 1)(), (ctypes.c_int64 * 4)()
    assert lib.ssd_jpeg_plan((L.SsdJpegInfo * 1)(info), 1, table, totals) == OK
    buf = np.zeros(4096, np.uint8)
    fake = buf.ctypes.data + (-buf.ctypes.data) % 16
    names = ("images_dev", "coef_dev", "quant_dev", "workspace_dev", "frames_dev")

    def call(B=1, **kw):
        a = dict({n: fake for n in names}, **kw)
        rc = lib.ssd_jpeg_decode(table, a["images_dev"], B, a["coef_dev"], a["quant_dev"], a["workspace_dev"], a["frames_dev"], None)
        return rc, lib.ssd_last_error().decode()

    def refused(word, **kw):
        rc, msg = call(**kw)
        assert rc == INVALID and msg == "ssd_jpeg_decode: " + word, (rc, msg)

    for name, align in zip(names, (8, 16, 16, 16, 16)):
        refused(name + " is NULL", **{name: None})
        refused("%s must be %d-byte aligned" % (name, align), **{name: fake + align // 2})
        refused("%s must be %d-byte aligned" % (name, align), **{name: fake + 1})
    refused("images_dev is NULL", **{n: None for n in names})                   # the first of the table is the one reported
    refused("coef_dev must be 16-byte aligned", coef_dev=fake + 8, frames_dev=None)
    assert call(B=0, **{n: None for n in names})[0] == OK
    assert lib.ssd_jpeg_decode(None, None, 0, None, None, None, None, None) == OK


# ----------------------------------------------------------------------------- the parser under the sanitizers
def test_parser_under_sanitizers_on_damaged_files(tmp_path):
    """tests/jpeg_host_check.cpp + csrc/jpeg_host.cpp alone, built with -fsanitize=address,undefined: every prefix and every
    single-byte change at each of the first 700 bytes of three files, the output buffers sized exactly as `info` says; and of two
    loud files (tests/helpers/jpeg_loud.py), whose blocks pass the block-sum screen and run the exact passes: one the rule pins,
    one it refuses."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "jpeg_host_check.cpp"), os.path.join(ROOT, "single-shot-detector_amd", "csrc", "jpeg_host.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and re.search(r"asan|ubsan|sanitize", built.stderr):
        pytest.skip("the sanitizer runtime is absent: %s" % built.stderr.strip().splitlines()[-1])
    assert built.returncode == 0, built.stderr
    from tests.helpers import jpeg_loud
    loud = {name: (blob, p) for name, blob, p in jpeg_loud.loud()}
    pinned, past = loud["loud-16x16-420-noise-v500"], loud["loud-16x16-420-noise-past-v"]
    assert jpeg_ref.pinned(pinned[1]) and not jpeg_ref.pinned(past[1])
    files = []
    for k, blob in enumerate((_base("420", 21, 19), _base("422", 8, 24, restart_marker_blocks=1, optimize=True), _base("gray", 16, 16, 30),
                              pinned[0], past[0])):
        path = str(tmp_path / ("f%d.jpg" % k))
        with open(path, "wb") as f:
            f.write(blob)
        files.append(path)
    run = subprocess.run([exe] + files[:4] + ["--refused"] + files[4:], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    counts = [int(v) for v in re.findall(r"runs (\d+)", run.stdout)]
    assert len(counts) == 5 and all(c > 700 for c in counts), run.stdout
    accepted = [int(v) for v in re.findall(r"accepted (\d+)", run.stdout)]
    assert len(accepted) == 5 and all(v > 0 for v in accepted[:4]), "the untouched file must decode"
    assert run.stdout.count(" refused\n") == 1 and run.stdout.splitlines()[4].endswith(" refused")
