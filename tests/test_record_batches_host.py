"""ssd.record_batches without a GPU: the one scatter of a mixed batch's records into the rows of a caller's block, driven by the
stand-in engine of tests/helpers/sharding_stub.py on CPU int32 tensors.  Every row is compared with the stub's record of that
frame, computed directly."""
import numpy as np
import torch

from tests.helpers import sharding_stub

T = 5
A, B = (40, 60), (100, 30)          # two network shapes of the stub: (64, 64) and (128, 64)
FILL = -7


class Engine(sharding_stub.StubEngine):
    """The stub, remembering every block it was asked for."""

    def __init__(self):
        super().__init__(T)
        self.fresh = []

    def new_records(self, B, dev):
        self.fresh.append(super().new_records(B, dev))
        return self.fresh[-1]


def frames_of(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in sizes]


def run(ssd, frames, max_batch, records, rows=None):
    """-> (the engine, [(part, the block enqueue received)...])."""
    eng, calls = Engine(), []

    def enqueue(part, block):
        calls.append((list(part), block))
        eng.forward_mixed_host([frames[i] for i in part], block)
    ssd.ssd.record_batches(eng, [f.shape[:2] for f in frames], max_batch, records, enqueue, rows)
    assert [p for p, _b in calls] == ssd.ssd.mixed_batches(eng, [f.shape[:2] for f in frames], max_batch)
    return eng, calls


def is_view_at(block, records, row):
    return (block.untyped_storage().data_ptr() == records.untyped_storage().data_ptr()
            and block.data_ptr() == records[row].data_ptr() and block.is_contiguous())


def check_rows(records, frames, rows):
    """Frame i's record in row rows[i]; every other row as it was filled."""
    for i, f in enumerate(frames):
        assert np.array_equal(records[rows[i]].numpy(), sharding_stub.record_of(f, T)), (i, rows[i])
    others = sorted(set(range(len(records))) - set(rows))
    assert bool((records[others] == FILL).all())


def block(n):
    return torch.full((n, 6 * T + 1), FILL, dtype=torch.int32)


def test_one_shape_writes_into_slices_of_the_block(ssd):
    frames, records = frames_of([A] * 7, 1), block(7)
    eng, calls = run(ssd, frames, 4, records)
    assert [p for p, _b in calls] == [[0, 1, 2, 3], [4, 5], [6]]
    assert all(is_view_at(b, records, p[0]) and len(b) == len(p) for p, b in calls) and eng.fresh == []
    check_rows(records, frames, list(range(7)))


def test_interleaved_shapes_go_through_a_fresh_block_to_their_rows(ssd):
    frames, records = frames_of([A, B, A, B, A, B, A], 2), block(7)
    eng, calls = run(ssd, frames, 2, records)
    assert [p for p, _b in calls] == [[0, 2], [4, 6], [1, 3], [5]]
    for p, b in calls:
        if p == [5]:
            assert is_view_at(b, records, 5)
        else:
            assert any(b is f for f in eng.fresh) and b.untyped_storage().data_ptr() != records.untyped_storage().data_ptr()
            assert tuple(b.shape) == (len(p), 6 * T + 1)
    assert len(eng.fresh) == 3
    check_rows(records, frames, list(range(7)))


def test_explicit_rows_leave_every_other_row_untouched(ssd):
    """Five frames into rows [7, 2, 3, 0, 5] of nine: (2, 3) is consecutive and ascending, (7, 0) is neither."""
    frames, records, rows = frames_of([B, A, A, B, B], 3), block(9), [7, 2, 3, 0, 5]
    eng, calls = run(ssd, frames, 2, records, rows)
    assert [p for p, _b in calls] == [[0, 3], [4], [1, 2]]
    assert not is_view_at(calls[0][1], records, 7) and len(eng.fresh) == 1
    assert is_view_at(calls[1][1], records, 5) and is_view_at(calls[2][1], records, 2)
    check_rows(records, frames, rows)


def test_no_frame_does_nothing(ssd):
    records = block(3)
    eng, calls = run(ssd, [], 4, records)
    assert calls == [] and eng.fresh == [] and bool((records == FILL).all())
    eng, calls = run(ssd, [], 4, records, [])
    assert calls == [] and eng.fresh == [] and bool((records == FILL).all())
