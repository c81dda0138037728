"""ssd_train_grad_pack / ssd_train_grad_reduce on the GPU (include/ssd_hip.h, "the TRAIN step's gradient exchange") against the
numpy float32 restatement of tests/helpers/train_reduce_ref.py, bit for bit (but for the sign of a NaN that inf - inf creates): every float of a slice (padding +0.0), every output
element, the losses and the weights; guard words behind every slice and around every output; two calls give the same bytes."""
import numpy as np
import pytest

from helpers import train_reduce_ref as ref

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = 0x7FA5A5A5                     # a NaN no arithmetic here produces; compared as an integer
GUARD = 8
# counts around a quad and around a block, an empty row, a NULL row, two rows of kind 1, and a row that holds a whole block
# (offsets 0 0 4 8 12 20 4116 8212 12312 12320 12452 16552: block 5 = bucket floats [20480, 24576) lies inside the last row)
COUNTS = (0, 1, 3, 4, 5, 4095, 4096, 4097, 7, 130, 4100, 9000)
KINDS = (0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0)
PRESENT = (1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1)
BOUNDARY = 20480 - 16552                  # the element of the last row that starts block 5


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _nan(payload):
    return np.array([0x7FC00000 | payload], np.uint32).view(f32)[0]


def _values(rng, counts, kinds, G):
    """x[r][t]: values over +-40 binades with the specials of the module's docstring planted."""
    x = [[(rng.standard_normal(n) * np.exp2(rng.uniform(-40, 40, n))).astype(f32) for n in counts] for _ in range(G)]
    for r in range(G):
        for t, n in enumerate(counts):
            if n >= 5:
                x[r][t][1] = f32(1e-40) * f32(r + 1)               # denormals, whose sums and products stay denormal
                x[r][t][2] = f32(-0.0)                             # -0.0 on every rank: the result is -0.0
            if kinds[t] == 1:
                x[r][t][:] = np.abs(x[r][t]) % f32(1e6)            # statistics: moderate, so that their plain sum is finite
    last = G - 1
    x[last][5][4094] = _nan(0x12345)                               # a NaN with a payload on ONE rank, on a row's last element
    x[0][7][0] = f32(-np.inf)                                      # -inf on a row's first element, one rank
    for r in range(G):
        x[r][6][4095] = f32(np.inf)                                # +inf on a row's last element, every rank: stays +inf
    x[last][11][BOUNDARY - 1] = _nan(0x00777)                      # the last float of block 4 ...
    x[0][11][BOUNDARY] = f32(np.inf)                               # ... and the first of block 5: +inf, and -inf on the next rank
    if G > 1:
        x[1][11][BOUNDARY] = f32(-np.inf)                          # inf - inf: a created NaN
    x[last][10][4099] = _nan(0x00042)                              # kind 1: a NaN on the last element
    return x


def _headers(rng, G, mode):
    n = rng.integers(1, 200, G).astype(f32)
    if mode == "one_zero":
        n[G // 2] = 0
    elif mode == "all_zero":
        n[:] = 0
    loc = rng.uniform(0.1, 3.0, G).astype(f32)
    cls = rng.uniform(0.1, 3.0, G).astype(f32)
    return np.stack([n, loc, cls], 1)


class _Placed:
    """A device tensor of n floats at 4-byte offset k inside a 16-byte group, at least GUARD sentinel words before and after it."""

    def __init__(self, cuda, n, k, host=None):
        self.n, self.k = n, k
        self.base = cuda.full((n + 2 * GUARD + 4,), SENTINEL, dtype=cuda.int32, device="cuda")
        assert self.base.data_ptr() % 16 == 0
        self.lo = GUARD + k                                        # GUARD is a multiple of 4: the tensor starts k words into a group
        self.view = self.base[self.lo:self.lo + n].view(cuda.float32)
        self.ptr = self.base.data_ptr() + 4 * self.lo
        assert self.ptr % 16 == 4 * k
        if host is not None and n:
            self.view.copy_(cuda.from_numpy(np.ascontiguousarray(host, dtype=f32)))

    def read(self):
        """(the tensor's uint32 bits, whether every guard word is intact)."""
        words = self.base.cpu().numpy().view(np.uint32)
        inside = words[self.lo:self.lo + self.n]
        outside = np.concatenate([words[:self.lo], words[self.lo + self.n:]])
        return inside, bool((outside == SENTINEL).all())


def _table(train_calls, cuda, counts, kinds, ptrs):
    rows = np.zeros(len(counts), train_calls.REDUCE_ROW_DTYPE)
    rows["count"], rows["kind"], rows["data"] = counts, kinds, ptrs
    rows["offset"] = ref.bucket_layout(counts)[0]
    host = cuda.from_numpy(rows.view(np.uint8).copy())
    return host, host.cuda()


def _exchange(cuda, counts, kinds, present, x, headers, k, twice=True):
    """Packs every rank's tensors, checks the gathered buffer against pack_ref, reduces (twice, into fresh outputs) and checks every
    output, the losses and the weights against reduce_ref.  Returns the outputs' bits."""
    from ssd_amd import train_calls
    G = len(x)
    slice_floats = ref.bucket_layout(counts)[2]
    assert train_calls.bucket_layout(counts)[1] == slice_floats
    flat = cuda.full((G * slice_floats + GUARD,), SENTINEL, dtype=cuda.int32, device="cuda")
    gathered = flat[:G * slice_floats].view(cuda.float32).view(G, slice_floats)
    keep = []
    for r in range(G):
        placed = [_Placed(cuda, n, k, x[r][t]) if present[t] else None for t, n in enumerate(counts)]
        rows_host, rows_dev = _table(train_calls, cuda, counts, kinds, [p.ptr if p is not None else 0 for p in placed])
        assert train_calls.train_bucket_floats(rows_host) == slice_floats
        train_calls.train_grad_pack(rows_host, rows_dev, cuda.from_numpy(headers[r]).cuda(), gathered[r])
        keep.append((placed, rows_host, rows_dev))
    cuda.cuda.synchronize()
    got = flat.cpu().numpy().view(np.uint32)
    assert (got[G * slice_floats:] == SENTINEL).all(), "pack wrote behind the last slice"
    want = np.stack([ref.pack_ref([x[r][t] if present[t] else None for t in range(len(counts))], counts, headers[r]) for r in range(G)])
    assert np.array_equal(got[:G * slice_floats].reshape(G, slice_floats), _bits(want)), "a slice differs from pack_ref"
    for r in range(G):                                             # pack only read the tensors
        for t, p in enumerate(keep[r][0]):
            if p is not None:
                inside, intact = p.read()
                assert intact and np.array_equal(inside, _bits(x[r][t])), (r, t)
    outs_want, losses_want, weights_want = ref.reduce_ref(want, counts, kinds, present)
    results = []
    for _ in range(2 if twice else 1):
        outs = [_Placed(cuda, n, k) if present[t] else None for t, n in enumerate(counts)]
        small = _Placed(cuda, 2 + G, 1)
        rows_host, rows_dev = _table(train_calls, cuda, counts, kinds, [p.ptr if p is not None else 0 for p in outs])
        train_calls.train_grad_reduce(rows_host, rows_dev, gathered, small.view[:2], small.view[2:])
        cuda.cuda.synchronize()
        bits = []
        for t, p in enumerate(outs):
            if p is None:
                bits.append(None)
                continue
            inside, intact = p.read()
            assert intact, "reduce wrote outside row %d (count %d)" % (t, counts[t])
            inside = ref.created_nans_as(inside, _bits(outs_want[t]))       # inf - inf: some NaN, its sign is not pinned
            differ = np.nonzero(inside != _bits(outs_want[t]))[0]
            assert len(differ) == 0, "row %d (count %d, kind %d): %d elements differ, first at %d: got %08x want %08x" % (
                t, counts[t], kinds[t], len(differ), differ[0], inside[differ[0]], _bits(outs_want[t])[differ[0]])
            bits.append(inside.copy())
        inside, intact = small.read()
        assert intact, "reduce wrote outside losses_out / weights_out"
        assert np.array_equal(inside[:2], _bits(losses_want)), (inside[:2].view(f32), losses_want)
        assert np.array_equal(inside[2:], _bits(weights_want)), (inside[2:].view(f32), weights_want)
        results.append(bits)
    assert (flat.cpu().numpy().view(np.uint32)[:G * slice_floats].reshape(G, slice_floats) == _bits(want)).all(), "reduce wrote to the gathered buffer"
    if twice:
        assert all(a is None or np.array_equal(a, b) for a, b in zip(*results)), "two calls gave different bytes"
    return results[0]


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_pack_and_reduce_match_the_restatement(cuda, G, k):
    """The table of COUNTS with data at 4-byte offset k inside a 16-byte group (k = 0: the 16-byte path; else element by element)."""
    rng = np.random.default_rng(100 * G + k)
    x = _values(rng, COUNTS, KINDS, G)
    headers = _headers(rng, G, "plain")
    bits = _exchange(cuda, COUNTS, KINDS, PRESENT, x, headers, k)
    if G == 1:                                                     # c_0 = 1.0f and 1.0f / 1: the identity
        for t in range(len(COUNTS)):
            if PRESENT[t]:
                assert np.array_equal(bits[t], _bits(x[0][t])), t
    else:
        t, i = 11, BOUNDARY
        assert bits[t][i] == 0x7FC00000 and np.isnan(bits[t][i - 1:i].view(f32)).all()
        assert bits[6][4095] == 0x7F800000 and bits[7][0] == 0xFF800000


@pytest.mark.parametrize("mode", ["one_zero", "all_zero"])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_headers_with_no_matches(cuda, G, mode):
    """One rank without a match (its weight is 1 / max(S, 1)) and every rank without one (every weight is 1.0f: a plain sum)."""
    rng = np.random.default_rng(7 * G + len(mode))
    x = _values(rng, COUNTS, KINDS, G)
    headers = _headers(rng, G, mode)
    want = ref.weights_ref(headers[:, 0])
    if mode == "all_zero":
        assert (want == 1).all()
    elif G > 1:
        assert want[G // 2] == f32(1) / headers[:, 0].sum(dtype=f32)
    bits = _exchange(cuda, COUNTS, KINDS, PRESENT, x, headers, 0, twice=False)
    if G == 1:
        assert all(np.array_equal(bits[t], _bits(x[0][t])) for t in range(len(COUNTS)) if PRESENT[t])


def test_a_table_past_one_grid_pass(cuda):
    """2 049 blocks at G = 2: the grid of 2 048 strides once more; a kind-1 row and a small row in front shift the big one off the
    block grid."""
    counts, kinds, present = (1001, 77, 2048 * 4096 + 100), (0, 1, 0), (1, 1, 1)
    assert ref.bucket_layout(counts)[1] == 2049 * 4096
    rng = np.random.default_rng(5)
    x = [[(rng.standard_normal(n) * np.exp2(rng.integers(-40, 40, n))).astype(f32) for n in counts] for _ in range(2)]
    for r in range(2):
        x[r][1] = np.abs(x[r][1]) % f32(1e6)
    x[1][2][-1] = _nan(0x321)
    x[0][2][2048 * 4096 - 1084 - 1] = f32(np.inf)                  # bucket floats 8388607 and 8388608: around the last block's start
    x[1][2][2048 * 4096 - 1084] = f32(-np.inf)
    _exchange(cuda, counts, kinds, present, x, _headers(rng, 2, "plain"), 0, twice=False)
