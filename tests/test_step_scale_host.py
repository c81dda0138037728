"""The premises of tests/test_gpu_step_scale.py, without a GPU: every table of helpers/step_scale_cases.py has the blocks, grid passes
and stage-2 chunks it was laid out for, its planted values sit where the case says, and the two tiled expectations (one row past
2^32 bytes for the norms and histograms, slices past 2^32 bytes for the gradient exchange) equal the full restatements at 40 periods."""
import numpy as np
import pytest

from helpers import histogram_ref as href
from helpers import step_scale_cases as cases
from helpers import train_norms_ref as nref
from helpers import train_reduce_ref as rref

f32 = np.float32
BLOCK, GRID, CHUNK = cases.BLOCK, cases.GRID, cases.CHUNK


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _last_block_elements(row):
    return len(row.w) + row.wo - (nref.n_blocks(len(row.w), row.wo) - 1) * BLOCK


def test_the_kernels_still_have_the_grid_and_the_chunk_the_cases_assume():
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "single-shot-detector_amd", "csrc")
    # the three files take the grid and the chunk from the one header, by these names, and define no grid of their own
    for name, words in (("train_table.h", ("TBL_MAX_GRID = 2048", "TBL_WAVE = 64", "blocks < TBL_MAX_GRID ? blocks : TBL_MAX_GRID")),
                        ("train_norms.hip", ('#include "train_table.h"', "grid_for(blocks)", "dim3(TBL_WAVE)", "base += TBL_WAVE")),
                        ("train_hist.hip", ('#include "train_table.h"', "grid_for(blocks)", "dim3(TBL_WAVE)", "base += TBL_WAVE")),
                        ("train_reduce.hip", ('#include "train_table.h"', "grid_for(blocks < 1 ? 1 : blocks)"))):
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        assert all(w in text for w in words), name
        assert name == "train_table.h" or "MAX_GRID =" not in text, name
    assert (GRID, CHUNK, BLOCK) == (2048, 64, 4096) and cases.passes(2048) == 1 and cases.passes(2049) == 2 and cases.passes(1) == 1


# ----------------------------------------------------------------------------- A
def test_a_sits_on_the_chunk_boundaries_inside_one_grid_pass():
    rows = cases.case_a()
    blocks = cases.row_blocks(rows)
    assert blocks == [63, 64, 65, 127, 128, 129, 256, 257, 1] and sum(blocks) == 1090 and cases.passes(sum(blocks)) == 1
    assert [cases.chunks(b) for b in blocks] == [1, 1, 2, 2, 2, 3, 4, 5, 1]
    assert [r.wo for r in rows[:8]] == [0, 1, 2, 3, 0, 1, 2, 3]
    assert [r.g is not None for r in rows] == [True, False] * 4 + [True] and all(r.decay == 1 for r in rows if r.g is not None)
    assert any(r.g is not None and r.go != r.wo for r in rows) and any(r.g is not None and r.go == r.wo for r in rows)
    # the rows whose last chunk ends on a one-element block, right behind a full chunk
    one = [b for r, b in zip(rows, blocks) if _last_block_elements(r) == 1]
    assert one == [65, 129, 257] and all((b - 1) % CHUNK == 0 for b in one)
    assert [_last_block_elements(r) for r in rows if nref.n_blocks(len(r.w), r.wo) % CHUNK == 0] == [BLOCK] * 3


def _block_of(row, i):
    return (i + row.wo) // BLOCK


@pytest.mark.parametrize("plane", ["w", "g"])
def test_a_plants_its_nans_and_extremes_in_the_named_blocks(plane):
    for row, nb in zip(cases.case_a()[:8], cases.A_BLOCKS):
        x = row.w if plane == "w" else row.g
        if x is None:
            continue
        nans = sorted({_block_of(row, i) for i in np.nonzero(np.isnan(x))[0]})
        big = cases.A_EXTREME[0 if plane == "w" else 1]
        lo, hi = _block_of(row, int(np.nanargmin(x))), _block_of(row, int(np.nanargmax(x)))
        assert np.nanmax(x) == big and (x == big).sum() == 1 and (x == -big).sum() == (1 if nb > CHUNK else 0)
        assert np.abs(x[np.isfinite(x) & (np.abs(x) != big)]).max() < 2.0 ** 44
        if nb <= CHUNK:                                              # no block 64: no planted minimum
            assert nans == [nb - 1] and hi == nb - 1                # one chunk: the NaN and the maximum in its last block
        elif nb == CHUNK + 1:                                        # block 64 is one element: one extreme there, the other in block 63
            assert nans == [CHUNK - 1] and {lo, hi} == {CHUNK - 1, CHUNK} and (lo == CHUNK) == (plane == "w")
        else:
            assert nans == [CHUNK - 1, CHUNK] and lo == CHUNK and hi == nb - 1


def test_a_has_a_row_that_overflows_only_through_the_decay_term():
    row = cases.case_a()[8]
    assert len(row.w) == BLOCK and row.wo == 0 and row.decay == 1 and np.isfinite(row.w).all() and np.isfinite(row.g).all()
    gp = href.gradient_plane(row.w, row.g, 1, cases.WD)
    assert sorted(gp[~np.isfinite(gp)].tolist()) == [-np.inf, np.inf]
    assert np.isfinite(href.gradient_plane(row.w, row.g, 0, cases.WD)).all()


# ----------------------------------------------------------------------------- B1
@pytest.mark.parametrize("views", [False, True], ids=["aligned", "views_at_1_2_3"])
@pytest.mark.parametrize("backbone", ["mobilenet", "shufflenet"])
def test_b1_takes_two_grid_passes(backbone, views):
    import ssd_amd
    from ssd_amd import train_step
    names, rows = cases.case_b1(backbone, views)
    assert list(names) == train_step.trainable_names(cases.BACKBONES[backbone]) and len(rows) == len(names)
    shapes = ssd_amd.synthetic_weights(cases.BACKBONES[backbone], seed=0)
    assert [len(r.w) for r in rows] == [shapes[n].size for n in names]
    total = sum(cases.row_blocks(rows))
    print("%s, views %r: %d tensors, %d blocks, the largest %d" % (backbone, views, len(rows), total, max(cases.row_blocks(rows))))
    assert 2049 <= total <= 4096 and cases.passes(total) == 2
    assert [r.wo for r in rows] == [1 + i % 3 if views else 0 for i in range(len(rows))]
    assert [r.decay for r in rows] == [int(train_step.decays(n)) for n in names] and 0 < sum(r.decay for r in rows) < len(rows)
    null = sum(r.g is None for r in rows)
    assert len(rows) // 20 <= null <= len(rows) // 5                 # about one in ten
    assert max(cases.chunks(b) for b in cases.row_blocks(rows)) >= 3


# ----------------------------------------------------------------------------- B2
def test_b2_takes_three_trips_on_300_hardware_blocks():
    rows = cases.case_b2()
    blocks, first = cases.row_blocks(rows), cases.first_blocks(rows)
    assert blocks == [lay[1] for lay in cases.B2_LAYOUT] and sum(blocks) == cases.B2_TOTAL == 2 * GRID + 300
    assert cases.passes(cases.B2_TOTAL) == 3 and cases.B2_TOTAL - 2 * GRID == cases.B2_THIRD
    spans = [(f, f + b) for f, b in zip(first, blocks)]
    for edge in (GRID, 2 * GRID):                                    # a row on either side of the start of the second and third pass
        assert any(lo <= edge - 1 and edge < hi for lo, hi in spans), edge
    empty = [t for t, r in enumerate(rows) if len(r.w) == 0]
    single = [t for t, r in enumerate(rows) if len(r.w) == 1]
    assert len(empty) == 1 and blocks[empty[0]] == 0 and first[empty[0]] >= GRID and rows[empty[0]].decay == 1
    assert len(single) == 1 and blocks[single[0]] == 1 and first[single[0]] >= GRID and single[0] == empty[0] + 1
    assert {r.wo for r in rows} == {0, 1, 2, 3} and any(r.g is None for r in rows)
    assert any(_last_block_elements(r) == 1 and len(r.w) > 1 for r in rows)


def test_b2_shows_every_third_trip_block_wide_then_constant_then_wide_values():
    """Hardware block h < 300 meets work blocks h, h + 2048 and h + 4096: many buckets in both planes, ONE bucket per plane (another
    one in the gradient plane than in w), many buckets again."""
    rows = cases.case_b2()
    first = cases.first_blocks(rows)

    def planes(c):
        t = cases.row_of_block(rows, c)
        lo, hi = cases.block_range(rows[t], c - first[t])
        r = rows[t]
        assert r.g is not None and hi > lo, (c, t)
        return cases.buckets(r.w[lo:hi]), cases.buckets(href.gradient_plane(r.w[lo:hi], r.g[lo:hi], r.decay, cases.WD)), hi - lo

    narrowest = 10 ** 9
    for h in range(cases.B2_THIRD):
        for c in (h, h + 2 * GRID):
            bw, bg, n = planes(c)
            if n >= 1000:
                narrowest = min(narrowest, len(bw), len(bg), bw.max() - bw.min(), bg.max() - bg.min())
            assert n >= 90, c
        bw, bg, n = planes(h + GRID)
        assert len(bw) == 1 and len(bg) == 1 and bw[0] != bg[0], h
    print("the narrowest wide block of the first and third trip: %d buckets" % narrowest)
    assert narrowest >= 400                                          # +-40 binades are some 580 buckets on either side of zero
    kinds = {cases.B2_LAYOUT[cases.row_of_block(rows, h + GRID)][0] for h in range(cases.B2_THIRD)}
    assert kinds == {"const"} and len({cases.row_of_block(rows, h + GRID) for h in range(cases.B2_THIRD)}) == 3


# ----------------------------------------------------------------------------- C
def test_c_plants_its_values_past_byte_offset_2_to_the_32():
    pw, tw, pg, tg = cases.case_c()
    assert cases.C_COUNT == 2 ** 30 + 3 * BLOCK + 5 and cases.C_PERIODS * BLOCK * 4 == 2 ** 32
    blocks = nref.n_blocks(cases.C_COUNT, 0)
    assert blocks == 2 ** 18 + 4 and cases.passes(blocks) == 129 and cases.chunks(blocks) == 4097 and blocks % CHUNK == 4
    assert cases.C_NEED <= 8.1 * cases.GIB < cases.C_FLOOR and cases.C_COUNT <= 2 ** 40
    for pattern, tail, key, big in ((pw, tw, "w", cases.A_EXTREME[0]), (pg, tg, "g", cases.A_EXTREME[1])):
        at = cases.C_PLANTED[key]
        assert all(4 * (cases.C_PERIODS * BLOCK + i) > 2 ** 32 for i in at) and len({i // BLOCK for i in at}) >= 3
        assert np.isnan(tail[at[0]]) and tail[at[1]] == -np.inf and tail[at[2]] == -big and tail[at[3]] == big
        assert (~np.isfinite(tail)).sum() == 2 and np.isfinite(pattern).all()          # each occurs nowhere else
        rest = np.delete(tail, list(at))
        assert max(np.abs(rest).max(), np.abs(pattern).max()) < 2.0 ** 44
    assert cases.C_PLANTED["w"][3] == cases.C_TAIL - 1               # the row's very last element is its maximum
    assert not set(cases.C_PLANTED["w"]) & set(cases.C_PLANTED["g"])


@pytest.mark.parametrize("decay", [0, 1])
def test_the_tiled_norms_and_histograms_are_the_restatements_at_40_periods(decay):
    pw, tw, pg, tg = cases.case_c()
    w, g = cases.tiled_row(pw, tw, 40), cases.tiled_row(pg, tg, 40)
    sums, bad = cases.tiled_norms(pw, tw, pg, tg, 40)
    want_s, want_b = nref.table_norms([(w, g, 0)])
    assert np.array_equal(sums.view(np.int64), want_s.view(np.int64)) and np.array_equal(bad, want_b) and bad.tolist() == [[2, 2]]
    counts, stats = cases.tiled_histograms(pw, tw, pg, tg, decay, cases.WD, 40)
    want_c, want_st = href.table_histograms([(w, g, 0, decay)], cases.WD)
    assert np.array_equal(counts, want_c) and stats.tobytes() == want_st.tobytes()
    assert stats["bad"].tolist() == [[2, 4 if decay else 2]] and (counts.sum(axis=2) == stats["num"]).all()


# ----------------------------------------------------------------------------- D1
def test_d1_names_every_instance_the_library_ships():
    import os
    from ssd_amd import train_calls
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "single-shot-detector_amd", "csrc", "train_reduce.hip")) as f:
        text = f.read()
    assert train_calls.REDUCE_MAX_RANKS == 16 and all("RED_CASE(%d)" % g in text for g in range(1, 17)) and "RED_CASE(17)" not in text


# ----------------------------------------------------------------------------- D2
def test_d2_is_a_run_of_small_rows_over_three_blocks():
    from ssd_amd import train_calls
    counts, kinds, present, marks = cases.d2_table()
    offsets, P, slice_floats = rref.bucket_layout(counts)
    theirs = train_calls.bucket_layout(counts)
    assert np.array_equal(theirs[0], offsets) and theirs[1] == slice_floats
    assert len(counts) == cases.D2_ROWS and max(counts) == 9 and min(counts) == 0 and P == 3 * BLOCK
    ends = [o + -(-n // 4) * 4 for o, n in zip(offsets, counts)]
    assert ends[-1] > 2 * BLOCK                                      # the rows span blocks 0, 1 and 2
    empty = [n == 0 for n in counts]
    assert 0.09 <= sum(empty) / len(counts) <= 0.16                  # roughly one in eight
    assert empty[:3] == [True] * 3 and not empty[3] and empty[-3:] == [True] * 3 and not empty[-4]
    # block 0 ends with a row, three empty rows share bucket float 4096 with the row that opens block 1
    e, z = marks["ends_block_0"], marks["empty_at_4096"]
    assert ends[e] == BLOCK and counts[e] > 0 and z == e + 1 and empty[z:z + 3] == [True] * 3 and counts[z + 3] > 0
    assert [offsets[t] for t in range(z, z + 4)] == [BLOCK] * 4 and present[e] and present[z + 3]
    # the start of block 2 falls inside a row
    s = marks["crosses_into_block_2"]
    assert offsets[s] < 2 * BLOCK < offsets[s] + counts[s] and present[s]
    # the neighbourhood of both boundaries is small rows
    for edge in (BLOCK, 2 * BLOCK):
        near = [n for o, n in zip(offsets, counts) if edge - 200 <= o <= edge + 200]
        assert len(near) >= 40 and max(near) <= 9
    null = [t for t, p in enumerate(present) if not p]
    assert 0.08 <= len(null) / len(counts) <= 0.1 and all(t % 10 == 9 for t in null)
    seen = [t for t, p in enumerate(present) if p]
    assert [t for t, k in enumerate(kinds) if k] == seen[6::7]
    x, at = cases.d2_values(np.random.default_rng(0), counts, kinds, present, cases.D2_G)
    assert len(set(at.values())) == 5 and all(present[t] for t in at.values())
    assert all(np.isfinite(x[r][t]).all() and (x[r][t] >= 0).all() and x[r][t].max(initial=0) < 1e6
               for r in range(cases.D2_G) for t, k in enumerate(kinds) if k and t != at["nan_kind1"])
    want = np.stack([rref.pack_ref([x[r][t] if present[t] else None for t in range(len(counts))], counts, [1, 2, 3]) for r in range(cases.D2_G)])
    outs, _losses, _weights = rref.reduce_ref(want, counts, kinds, present)
    assert _bits(outs[at["created"]])[-1] == rref.CREATED_NAN and _bits(outs[at["neg_zero"]])[-1] == 0x80000000
    assert _bits(outs[at["nan"]])[-1] != rref.CREATED_NAN and np.isnan(outs[at["nan"]][-1]) and outs[at["inf"]][-1] == np.inf


# ----------------------------------------------------------------------------- D3
def test_d3_puts_a_row_off_the_block_grid_past_2_to_the_32_bytes():
    from ssd_amd import train_calls
    counts = cases.d3_counts(cases.D3_PERIODS)
    assert counts == (3, 2 ** 30 + BLOCK + 5) and counts[1] <= 2 ** 40
    offsets, P, slice_floats = rref.bucket_layout(counts)
    theirs = train_calls.bucket_layout(counts)
    assert np.array_equal(theirs[0], offsets) and theirs[1] == slice_floats
    assert offsets == [0, 4] and P == 2 ** 30 + 2 * BLOCK and slice_floats * 4 > 2 ** 32 and cases.D3_HEAD == 16 + offsets[1]
    assert cases.passes(P // BLOCK) == 129
    # the planted values: in the tensors, in either rank's slice and (rank 1) in the gathered buffer past byte offset 2^32
    for i in (cases.D3_NAN_AT, cases.D3_INF_AT):
        at = cases.D3_PERIODS * BLOCK + i
        assert 4 * at > 2 ** 32 and 4 * (cases.D3_HEAD + at) > 2 ** 32 and i < cases.D3_TAIL
    ranks = cases.case_d3()
    assert len(ranks) == cases.D3_G == 2 and not np.array_equal(ranks[0][1], ranks[1][1])
    assert _bits(ranks[1][2])[cases.D3_NAN_AT] == 0x7FC54321 and np.isfinite(ranks[0][2][cases.D3_NAN_AT])
    assert ranks[0][2][cases.D3_INF_AT] == np.inf and ranks[1][2][cases.D3_INF_AT] == -np.inf
    assert all(np.isfinite(p).all() and np.isfinite(f).all() for f, p, _t in ranks)
    assert cases.D3_G * 4 * slice_floats + cases.D3_G * 4 * counts[1] <= cases.D3_NEED + cases.GIB // 8 < cases.D3_FLOOR


def test_the_tiled_exchange_is_the_restatement_at_40_periods():
    ranks = cases.case_d3()
    headers = np.array([[5, 0.25, 1.5], [9, 2.0, 0.125]], f32)
    counts, kinds, present = cases.d3_counts(40), (0, 0), (1, 1)
    full = np.stack([rref.pack_ref([f, cases.tiled_row(p, t, 40)], counts, headers[r]) for r, (f, p, t) in enumerate(ranks)])
    for r, (f, p, t) in enumerate(ranks):
        head, period, rest = cases.d3_tiled_pack(f, p, t, headers[r])
        assert len(head) == cases.D3_HEAD and len(rest) == 2 * BLOCK - 4
        assert np.array_equal(_bits(np.concatenate([head, np.tile(period, 40), rest])), _bits(full[r]))
    want, losses, weights = rref.reduce_ref(full, counts, kinds, present)
    two = np.stack([rref.pack_ref([f, cases.tiled_row(p, t, 2)], cases.d3_counts(2), headers[r]) for r, (f, p, t) in enumerate(ranks)])
    outs2, losses2, weights2 = rref.reduce_ref(two, cases.d3_counts(2), kinds, present)
    assert np.array_equal(_bits(cases.d3_tiled_reduce(outs2[1], 40)), _bits(want[1])) and np.array_equal(_bits(outs2[0]), _bits(want[0]))
    assert np.array_equal(_bits(losses), _bits(losses2)) and np.array_equal(_bits(weights), _bits(weights2))
    tail = _bits(want[1])[40 * BLOCK:]
    assert tail[cases.D3_INF_AT] == rref.CREATED_NAN and np.isnan(want[1][40 * BLOCK + cases.D3_NAN_AT])
