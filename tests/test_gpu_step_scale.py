"""ssd_train_norms, ssd_train_histograms and the gradient exchange past their easy paths, bit for bit against the numpy restatements
(helpers/train_norms_ref.py, histogram_ref.py, train_reduce_ref.py) through the runners of test_gpu_train_norms.py,
test_gpu_train_histograms.py and test_gpu_train_reduce.py: outputs and workspaces pre-filled with 0xFF bytes behind guards, no tolerance
anywhere (a NaN that inf - inf creates in the reduce is "some NaN").  The cases and their premises: helpers/step_scale_cases.py,
tests/test_step_scale_host.py.

  A   stage 2 at its chunk boundaries: rows of 63, 64, 65, 127, 128, 129, 256 and 257 blocks inside one grid pass
  B1  the whole trainable set of MobileNet and ShuffleNet in one launch: two grid passes
  B2  2 * 2048 + 300 blocks: three trips, every third-trip block meets wide values, a constant tensor, wide values
  C   one row of 2^30 + 3 * 4096 + 5 elements built on the device, its special values past byte offset 2^32
  D1  grad_reduce<G> for every G = 1 .. 16
  D2  1 500 rows of 0 .. 9 elements with runs of empty rows on the block boundaries
  D3  slices past 2^32 bytes at G = 2, the big row off the block grid"""
import time

import numpy as np
import pytest

import test_gpu_train_histograms as hist
import test_gpu_train_norms as norms
import test_gpu_train_reduce as red
from helpers import step_scale_cases as cases
from helpers import train_reduce_ref as rref
from test_gpu_train_histograms import limits_dev                     # noqa: F401  (that module's fixture)

pytestmark = pytest.mark.gpu

f32 = np.float32
BLOCK, CHUNK = cases.BLOCK, cases.CHUNK
UNSET = -2 ** 31                                                     # ssd_set_option's "unset"


def _i64(a):
    return np.ascontiguousarray(a).view(np.int64)


def _norms_cross_check(ssd, cuda, table, s):
    """sum_squares of every w plane has ssd_train_norms' bits (as the forty-tensor test of test_gpu_train_histograms.py)."""
    host, devrows, _arena = table
    T = host.numel() // ssd.train_calls.ROW_BYTES
    sums = cuda.empty((T, 2), dtype=cuda.float64, device="cuda")
    bad = cuda.empty((T, 2), dtype=cuda.int64, device="cuda")
    ssd.train_calls.train_norms(host, devrows, sums, bad)
    assert np.array_equal(_i64(s["sum_squares"][:, 0]), _i64(sums.cpu().numpy()[:, 0]))
    assert np.array_equal(s["bad"][:, 0], bad.cpu().numpy()[:, 0])


# ============================================================================= A. stage 2 at its chunk boundaries
def _a_planted_nans():
    return [1 if nb <= CHUNK + 1 else 2 for nb in cases.A_BLOCKS]


def test_a_norms_at_the_chunk_boundaries_of_stage_2(ssd, cuda):
    rows = cases.case_a()
    s, b = norms._run_and_check(ssd, cuda, cases.norms_specs(rows), "A")
    nans = _a_planted_nans()
    assert b[:8, 0].tolist() == nans and b[8].tolist() == [0, 0]
    assert b[:8, 1].tolist() == [n if r.g is not None else 0 for n, r in zip(nans, rows)]
    assert (s[:, 0] >= 2.0 ** 90).all() and np.isfinite(s).all()     # every row's planted maximum is in its sum


def test_a_histograms_at_the_chunk_boundaries_of_stage_2(ssd, cuda, limits_dev):  # noqa: F811
    rows = cases.case_a()
    c, s, table = hist._run_and_check(ssd, cuda, limits_dev, cases.hist_specs(rows), "A", weight_decay=cases.WD)
    _norms_cross_check(ssd, cuda, table, s)
    nans = _a_planted_nans()
    assert s["bad"][:8, 0].tolist() == nans and s["bad"][8].tolist() == [0, 2]      # the decay term alone overflows row 8's plane
    big = cases.A_EXTREME[0]
    assert (s["max"][:8, 0] == big).all() and [m == -big for m in s["min"][:8, 0]] == [nb > CHUNK for nb in cases.A_BLOCKS]
    assert (c.sum(axis=2) + s["bad"] == [[len(r.w), len(r.w) if r.g is not None else 0] for r in rows]).all()


# ============================================================================= B. past one and two grid passes
@pytest.mark.parametrize("kernel", ["norms", "histograms"])          # varies fastest: both kernels share one drawn table
@pytest.mark.parametrize("backbone", ["mobilenet", "shufflenet"])
@pytest.mark.parametrize("views", [False, True], ids=["aligned", "views_at_1_2_3"])
def test_b1_the_whole_trainable_set_in_two_grid_passes(ssd, cuda, limits_dev, kernel, backbone, views):  # noqa: F811
    """Every trainable tensor of the architecture in one launch (3 218 .. 3 664 blocks: the grid of 2 048 strides once more), about
    one in ten without a gradient; `views`: tensor i starts 1 + i % 3 floats past a 16-byte boundary."""
    _names, rows = cases.case_b1(backbone, views)
    tag = "B1 %s %s" % (backbone, "views" if views else "aligned")
    if kernel == "norms":
        s, b = norms._run_and_check(ssd, cuda, cases.norms_specs(rows), tag)
        assert not b.any() and (s[:, 0] > 0).all()
        assert ((s[:, 1] > 0) == [r.g is not None for r in rows]).all()
    else:
        c, s, table = hist._run_and_check(ssd, cuda, limits_dev, cases.hist_specs(rows), tag, weight_decay=cases.WD)
        _norms_cross_check(ssd, cuda, table, s)
        assert not s["bad"].any() and (c.sum(axis=2) == [[len(r.w), len(r.w) if r.g is not None else 0] for r in rows]).all()


def test_b2_norms_over_three_trips_of_the_grid(ssd, cuda):
    rows = cases.case_b2()
    s, b = norms._run_and_check(ssd, cuda, cases.norms_specs(rows), "B2")
    empty = [t for t, r in enumerate(rows) if len(r.w) == 0][0]
    assert not b.any() and s[empty].tolist() == [0.0, 0.0]
    for t, (cw, cg) in cases.B2_CONSTANTS.items():                   # a constant tensor's sums, block by block in double
        assert s[t, 0] > 0 and abs(s[t, 0] / (len(rows[t].w) * float(f32(cw)) ** 2) - 1) < 1e-9


@pytest.mark.parametrize("scheme", [None, 0])
def test_b2_histograms_meet_wide_constant_and_wide_blocks_in_turn(ssd, cuda, limits_dev, scheme):  # noqa: F811
    """Hardware block h < 300 flushes a wide range of buckets, then runs a constant tensor's block, then a wide one again: a bucket
    left in its LDS histogram, or a touched range one bucket short, lands in another tensor's counts."""
    rows = cases.case_b2()
    ssd.set_option("hist_scheme", UNSET if scheme is None else scheme)
    try:
        c, s, table = hist._run_and_check(ssd, cuda, limits_dev, cases.hist_specs(rows), "B2 scheme %r" % (scheme,), weight_decay=cases.WD)
    finally:
        ssd.set_option("hist_scheme", UNSET)
    assert (c.sum(axis=2) == s["num"]).all() and not s["bad"].any()
    assert (s["num"] == [[len(r.w), len(r.w) if r.g is not None else 0] for r in rows]).all()
    for t in cases.B2_CONSTANTS:                                     # one bucket per plane, and not the same one
        assert np.count_nonzero(c[t, 0]) == 1 and np.count_nonzero(c[t, 1]) == 1 and np.argmax(c[t, 0]) != np.argmax(c[t, 1])
    _norms_cross_check(ssd, cuda, table, s)


# ============================================================================= C. elements past 2^32 bytes
def _require_free(cuda, floor, need, what):
    """Fails -- it does not skip -- when less than `floor` bytes of device memory are free; prints the figure."""
    cuda.cuda.empty_cache()
    free, total = cuda.cuda.mem_get_info()
    print("%s: %.2f GiB of device memory free of %.2f GiB; the test holds %.2f GiB at its peak and asks for %.0f GiB free"
          % (what, free / cases.GIB, total / cases.GIB, need / cases.GIB, floor / cases.GIB))
    if free < floor:
        pytest.fail("%s holds %.1f GiB of device memory and asks for %.0f GiB to be free; only %.1f GiB are"
                    % (what, need / cases.GIB, floor / cases.GIB, free / cases.GIB))


def _words(cuda, host):
    """A host float32 array's bits on the device, as int32."""
    return cuda.from_numpy(np.ascontiguousarray(host, dtype=f32).view(np.int32).copy()).cuda()


def _tiled_on_device(cuda, pattern, tail, periods):
    """The pattern `periods` times and the tail behind it, built on the device: only the two small arrays cross to it."""
    n = periods * BLOCK
    t = cuda.empty(n + len(tail), dtype=cuda.float32, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[:n].view(periods, BLOCK).copy_(cuda.from_numpy(pattern).cuda())
    t[n:].copy_(cuda.from_numpy(tail))
    return t


def _first_wrong_period(cuda, words, period_words, periods):
    """words: int32 device view of periods * 4096 words -> None where every period has period_words' bits, else the first period of
    the slab of 16 384 that holds a differing one.  Compared on the device, slab by slab."""
    step = 2 ** 14
    for lo in range(0, periods, step):
        hi = min(periods, lo + step)
        if not bool((words[lo * BLOCK:hi * BLOCK].view(hi - lo, BLOCK) == period_words).all()):
            return lo
    return None


def _assert_tiled(cuda, tensor, pattern, tail, periods, what):
    n = periods * BLOCK
    bad = _first_wrong_period(cuda, tensor[:n].view(cuda.int32), _words(cuda, pattern), periods)
    assert bad is None, "%s: a period in [%d, %d) lost its bits" % (what, bad, bad + 2 ** 14)
    assert np.array_equal(tensor[n:].cpu().numpy().view(np.uint32), np.ascontiguousarray(tail, dtype=f32).view(np.uint32)), what + ": the tail"


def _guards_intact(raw, lead, inner):
    r = raw.reshape(-1).cpu().numpy()
    return bool((r[:lead] == hist.GUARD).all() and (r[lead + inner:] == hist.GUARD).all())


class _BigRow:
    """Case C's table on the device: one decaying row of C_COUNT elements at w offset 0, its gradient a second buffer."""

    def __init__(self, ssd, cuda, what):
        from ssd_amd import train_step
        _require_free(cuda, cases.C_FLOOR, cases.C_NEED, what)
        self.host_arrays = pw, tw, pg, tg = cases.case_c()
        t0 = time.perf_counter()
        self.w = _tiled_on_device(cuda, pw, tw, cases.C_PERIODS)
        self.g = _tiled_on_device(cuda, pg, tg, cases.C_PERIODS)
        cuda.cuda.synchronize()
        self.seconds = {"allocate and fill": time.perf_counter() - t0}
        rows = np.zeros(1, train_step.TENSOR_DTYPE)
        rows["w"] = rows["m"] = rows["v"] = rows["ema"] = self.w.data_ptr()      # m, v and ema are validated, never dereferenced
        rows["grad"], rows["count"], rows["decay"] = self.g.data_ptr(), cases.C_COUNT, 1
        rows["first_block"], self.blocks = train_step.block_starts(rows["w"], rows["count"])
        assert self.w.numel() == cases.C_COUNT == self.g.numel() and self.blocks == cases.C_PERIODS + 4
        self.host = cuda.from_numpy(rows.view(np.uint8).copy())
        self.dev = self.host.cuda()
        self.what = what

    def workspace(self, cuda, need):
        raw = cuda.full((need + 32,), hist.GUARD, dtype=cuda.uint8, device="cuda")
        ws = raw[16:16 + need]
        ws.fill_(hist.NAN_BYTE)
        assert ws.data_ptr() % 16 == 0
        return raw, ws

    def timed(self, cuda, key, t0):
        cuda.cuda.synchronize()
        self.seconds[key] = time.perf_counter() - t0

    def finish(self, cuda):
        t0 = time.perf_counter()
        pw, tw, pg, tg = self.host_arrays
        _assert_tiled(cuda, self.w, pw, tw, cases.C_PERIODS, "w")    # w and grad keep their bits
        _assert_tiled(cuda, self.g, pg, tg, cases.C_PERIODS, "grad")
        self.timed(cuda, "inputs unchanged", t0)
        print("%s: %s" % (self.what, ", ".join("%s %.3f s" % kv for kv in self.seconds.items())))


def test_c_norms_of_a_row_past_4_gib(ssd, cuda):
    """One row of 2^30 + 3 * 4096 + 5 elements (262 148 blocks: 129 trips of the grid, 4 097 chunks of stage 2).  The tail, past byte
    offset 2^32, holds the row's only NaN and -inf: an offset that wrapped at 32 bits reads pattern floats instead and shows in `bad`
    and in the sums.  Expected: the pattern block's partial added 2^18 times one by one, then the tail's (tiled_norms; equal to the
    restatement at 40 periods, test_step_scale_host.py)."""
    big = _BigRow(ssd, cuda, "C norms")
    calls = ssd.train_calls
    need = calls.train_norms_workspace_bytes(big.host)
    assert need == 32 * big.blocks
    sraw, sums = norms._guarded(cuda, (1, 2), cuda.float64)
    braw, bad = norms._guarded(cuda, (1, 2), cuda.int64)
    wraw, ws = big.workspace(cuda, need)
    t0 = time.perf_counter()
    calls.train_norms(big.host, big.dev, sums, bad, workspace=ws)
    big.timed(cuda, "ssd_train_norms", t0)
    t0 = time.perf_counter()
    want_s, want_b = cases.tiled_norms(*big.host_arrays, cases.C_PERIODS)
    big.seconds["tiled expectation (host)"] = time.perf_counter() - t0
    s, b = sums.cpu().numpy(), bad.cpu().numpy()
    print("C norms: sums %r, bad %r" % (s.tolist(), b.tolist()))
    assert np.array_equal(b, want_b) and b.tolist() == [[2, 2]], (b, want_b)
    assert np.array_equal(_i64(s), _i64(want_s)), (s, want_s)
    assert _guards_intact(sraw, 16, 16) and _guards_intact(braw, 16, 16) and _guards_intact(wraw, 16, need)
    big.finish(cuda)


def test_c_histograms_of_a_row_past_4_gib(ssd, cuda, limits_dev):  # noqa: F811
    """The same row, decaying: counts are 2^18 * counts(pattern) + counts(tail), the sums go block by block, and the row's minimum and
    maximum (each planted once, in the tail) come back in min and max."""
    big = _BigRow(ssd, cuda, "C histograms")
    calls = ssd.train_calls
    NB = len(ssd.histogram_limits())
    need = calls.train_histograms_workspace_bytes(big.host)
    assert need == 64 * big.blocks
    craw, counts = hist._guarded(cuda, (1, 2, NB), cuda.int64)
    sraw, stats = hist._guarded(cuda, (1, 2, 40), cuda.uint8)
    wraw, ws = big.workspace(cuda, need)
    t0 = time.perf_counter()
    calls.train_histograms(big.host, big.dev, cases.WD, limits_dev, counts, stats, workspace=ws)
    big.timed(cuda, "ssd_train_histograms", t0)
    t0 = time.perf_counter()
    want_c, want_s = cases.tiled_histograms(*big.host_arrays, 1, cases.WD, cases.C_PERIODS)
    big.seconds["tiled expectation (host)"] = time.perf_counter() - t0
    c, s = counts.cpu().numpy(), hist._host_stats(stats)
    print("C histograms: stats %r" % (s.tolist(),))
    hist._compare("C", c, s, want_c, want_s)
    assert (c.sum(axis=2) == s["num"]).all() and (s["num"] + s["bad"] == cases.C_COUNT).all() and s["bad"].tolist() == [[2, 4]]
    assert s["min"][0, 0] == -cases.A_EXTREME[0] and s["max"][0, 0] == cases.A_EXTREME[0]
    assert _guards_intact(craw, 2 * NB * 8, 2 * NB * 8) and _guards_intact(sraw, 80, 80) and _guards_intact(wraw, 16, need)
    big.finish(cuda)


# ============================================================================= D. the gradient exchange
@pytest.mark.parametrize("G", range(1, 17))
def test_d1_every_instance_of_grad_reduce(cuda, G):
    """The table of test_gpu_train_reduce.py at every G the library instantiates (that file runs G = 1, 2, 3 and 8)."""
    rng = np.random.default_rng(1000 + G)
    x = red._values(rng, red.COUNTS, red.KINDS, G)
    bits = red._exchange(cuda, red.COUNTS, red.KINDS, red.PRESENT, x, red._headers(rng, G, "plain"), 0, twice=False)
    if G == 1:
        assert all(np.array_equal(bits[t], red._bits(x[0][t])) for t in range(len(red.COUNTS)) if red.PRESENT[t])
    else:
        assert bits[11][red.BOUNDARY] == 0x7FC00000 and bits[6][4095] == 0x7F800000 and bits[7][0] == 0xFF800000


@pytest.mark.parametrize("G", [5, 11, 16])
def test_d1_one_rank_without_a_match(cuda, G):
    rng = np.random.default_rng(2000 + G)
    x = red._values(rng, red.COUNTS, red.KINDS, G)
    headers = red._headers(rng, G, "one_zero")
    assert rref.weights_ref(headers[:, 0])[G // 2] == f32(1) / headers[:, 0].sum(dtype=f32)
    red._exchange(cuda, red.COUNTS, red.KINDS, red.PRESENT, x, headers, 0, twice=False)


@pytest.mark.parametrize("k", [0, 2])
def test_d2_a_table_of_many_small_rows(cuda, k):
    """1 500 rows of 0 .. 9 elements over three blocks: the blocks walk hundreds of rows each, and the row search lands on a run of empty
    rows at bucket float 4096 and inside a row at 8192."""
    counts, kinds, present, _marks = cases.d2_table()
    rng = np.random.default_rng(3000 + k)
    x, at = cases.d2_values(rng, counts, kinds, present, cases.D2_G)
    bits = red._exchange(cuda, counts, kinds, present, x, red._headers(rng, cases.D2_G, "plain"), k, twice=False)
    assert bits[at["created"]][-1] == 0x7FC00000 and bits[at["neg_zero"]][-1] == 0x80000000 and bits[at["inf"]][-1] == 0x7F800000
    assert np.isnan(bits[at["nan"]][-1:].view(f32)).all() and np.isnan(bits[at["nan_kind1"]][-1:].view(f32)).all()


def test_d3_slices_past_4_gib(cuda):
    """G = 2, a 3-float row and one row of 2^30 + 4096 + 5 elements at bucket float 4: each slice is 4 GiB and 32 KiB, rank 1's lies
    wholly past byte offset 2^32 of the gathered buffer.  The two-period version of the same table goes through _exchange (pack_ref,
    reduce_ref); the big slices must hold its head, its period 2^18 times and its rest, the big output its reduced period 2^18 times
    and its reduced tail (d3_tiled_pack / d3_tiled_reduce: equal to the restatement at 40 periods, test_step_scale_host.py)."""
    from ssd_amd import train_calls
    _require_free(cuda, cases.D3_FLOOR, cases.D3_NEED, "D3")
    G, periods, n = cases.D3_G, cases.D3_PERIODS, cases.D3_PERIODS * BLOCK
    ranks = cases.case_d3()
    rng = np.random.default_rng(4000)
    headers = red._headers(rng, G, "plain")
    kinds, present = (0, 0), (1, 1)
    seconds = {}
    # the two-period table against the restatement
    t0 = time.perf_counter()
    counts2 = cases.d3_counts(2)
    x2 = [[front, cases.tiled_row(pattern, tail, 2)] for front, pattern, tail in ranks]
    bits2 = red._exchange(cuda, counts2, kinds, present, x2, headers, 0, twice=False)
    want2 = np.stack([rref.pack_ref(x2[r], counts2, headers[r]) for r in range(G)])
    _outs2, losses_want, weights_want = rref.reduce_ref(want2, counts2, kinds, present)
    period_out, tail_out = bits2[1][:BLOCK], bits2[1][2 * BLOCK:]
    assert np.array_equal(period_out, bits2[1][BLOCK:2 * BLOCK]) and tail_out[cases.D3_INF_AT] == rref.CREATED_NAN
    seconds["two-period exchange"] = time.perf_counter() - t0
    # pack
    counts = cases.d3_counts(periods)
    slice_floats = rref.bucket_layout(counts)[2]
    assert train_calls.bucket_layout(counts)[1] == slice_floats
    t0 = time.perf_counter()
    flat = cuda.full((G * slice_floats + red.GUARD,), red.SENTINEL, dtype=cuda.int32, device="cuda")
    gathered = flat[:G * slice_floats].view(cuda.float32).view(G, slice_floats)
    inputs = [_tiled_on_device(cuda, pattern, tail, periods) for _front, pattern, tail in ranks]
    fronts = [red._Placed(cuda, cases.D3_FRONT, 0, front) for front, _pattern, _tail in ranks]
    cuda.cuda.synchronize()
    seconds["allocate and fill"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    keep = []
    for r in range(G):
        rows_host, rows_dev = red._table(train_calls, cuda, counts, kinds, [fronts[r].ptr, inputs[r].data_ptr()])
        assert train_calls.train_bucket_floats(rows_host) == slice_floats
        train_calls.train_grad_pack(rows_host, rows_dev, cuda.from_numpy(headers[r]).cuda(), gathered[r])
        keep.append((rows_host, rows_dev))
    cuda.cuda.synchronize()
    seconds["ssd_train_grad_pack x 2"] = time.perf_counter() - t0

    def slices_are_tiled(when):
        assert bool((flat[G * slice_floats:] == red.SENTINEL).all()), when + ": a write behind the last slice"
        for r, (front, pattern, tail) in enumerate(ranks):
            head, period, rest = cases.d3_tiled_pack(front, pattern, tail, headers[r])
            got = gathered[r].view(cuda.int32)
            assert np.array_equal(got[:cases.D3_HEAD].cpu().numpy().view(np.uint32), red._bits(head)), (when, r, "head")
            bad = _first_wrong_period(cuda, got[cases.D3_HEAD:cases.D3_HEAD + n], _words(cuda, period), periods)
            assert bad is None, "%s: slice %d differs from the packed period in periods [%d, %d)" % (when, r, bad, bad + 2 ** 14)
            assert np.array_equal(got[cases.D3_HEAD + n:].cpu().numpy().view(np.uint32), red._bits(rest)), (when, r, "rest")

    t0 = time.perf_counter()
    slices_are_tiled("after pack")
    for r, (front, pattern, tail) in enumerate(ranks):              # pack only read the tensors
        _assert_tiled(cuda, inputs[r], pattern, tail, periods, "rank %d's big row" % r)
        inside, intact = fronts[r].read()
        assert intact and np.array_equal(inside, red._bits(front)), r
    seconds["compare the slices and the inputs"] = time.perf_counter() - t0
    # reduce, the output in the inputs' place
    del inputs
    t0 = time.perf_counter()
    out = red._Placed(cuda, counts[1], 0)
    out_front = red._Placed(cuda, cases.D3_FRONT, 0)
    small = red._Placed(cuda, 2 + G, 1)
    rows_host, rows_dev = red._table(train_calls, cuda, counts, kinds, [out_front.ptr, out.ptr])
    cuda.cuda.synchronize()
    seconds["allocate the output"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    train_calls.train_grad_reduce(rows_host, rows_dev, gathered, small.view[:2], small.view[2:])
    cuda.cuda.synchronize()
    seconds["ssd_train_grad_reduce"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    assert bool((out.base[:out.lo] == red.SENTINEL).all()) and bool((out.base[out.lo + out.n:] == red.SENTINEL).all()), "reduce wrote outside the big row"
    words = out.base[out.lo:out.lo + out.n]
    bad = _first_wrong_period(cuda, words[:n], cuda.from_numpy(period_out.view(np.int32).copy()).cuda(), periods)
    assert bad is None, "the output differs from the reduced period in periods [%d, %d)" % (bad, bad + 2 ** 14)
    tail = rref.created_nans_as(words[n:].cpu().numpy().view(np.uint32), tail_out)
    differ = np.nonzero(tail != tail_out)[0]
    assert len(differ) == 0, "the tail: %d elements differ, first at %d: got %08x want %08x" % (len(differ), differ[0], tail[differ[0]], tail_out[differ[0]])
    assert tail[cases.D3_INF_AT] == rref.CREATED_NAN and np.isnan(tail[cases.D3_NAN_AT:cases.D3_NAN_AT + 1].view(f32)).all()
    inside, intact = out_front.read()
    assert intact and np.array_equal(inside, bits2[0])
    inside, intact = small.read()
    assert intact, "reduce wrote outside losses_out / weights_out"
    assert np.array_equal(inside[:2], red._bits(losses_want)) and np.array_equal(inside[2:], red._bits(weights_want))
    slices_are_tiled("after reduce")                                 # reduce only read the gathered buffer
    seconds["compare the output and the slices"] = time.perf_counter() - t0
    print("D3: %s" % ", ".join("%s %.3f s" % kv for kv in seconds.items()))
