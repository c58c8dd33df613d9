"""The aligner in checkpointed memory (rmr_duplex_align_mode, csrc/k_duplex.hip: one kept DP line per strip, the trace recomputed one
strip at a time while walking back) against the full-trace form: every field and the bytes of every alignment's runs are equal,
whatever the mode and however the budget groups the batch; an alignment over the budget with its trace aligns all the same."""
import numpy as np
import pytest

import duplex_restate as R
from test_gpu_duplex_align import _as_dict, _grid_pairs, _mutate, _random, fixture_alignments

pytestmark = pytest.mark.gpu

FIELDS = ("status", "score", "end_row", "query_start", "ref_start", "ref_end", "n_runs")


def _extra_pairs():
    """A six-strip pair; the same with a simplex tail (the end row two strips above the last strip: the walk starts there); with a
    free simplex prefix; a path without a match operation."""
    rng = np.random.default_rng(12)
    duplex = _random(rng, 2600)
    simplex = _mutate(rng, duplex)
    assert 5 * 512 < len(simplex) <= 6 * 512
    return [(simplex, duplex), (simplex + _random(rng, 1300), duplex), (_random(rng, 700) + simplex, duplex), ("A", "CCCCCCCC")]


def _same(got, want, n):
    for k in FIELDS:
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    for a in range(n):
        assert got.words[got.run_off[a]:got.run_off[a] + got.n_runs[a]].tobytes() == \
            want.words[want.run_off[a]:want.run_off[a] + want.n_runs[a]].tobytes(), a


@pytest.fixture(scope="module")
def grid():
    """(pairs, the full-trace result, the checkpointed result): the grid of test_gpu_duplex_align and the extra pairs, ONE call each."""
    import torch

    from remora_amd import duplex_utils as DU

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    pairs = _grid_pairs() + _extra_pairs()
    return pairs, DU.align_batch(pairs), DU.align_batch(pairs, mode="checkpoint")


def test_grid_equals_the_full_trace_and_the_restatement(grid):
    from remora_amd import duplex_utils as DU

    pairs, full, ckpt = grid
    assert full.n_groups == 1 and full.n_checkpointed == 0
    assert ckpt.n_groups == 1 and ckpt.n_checkpointed == len(pairs)  # no pair of the grid is refused on the host
    assert full.status[-1] == DU.STATUS_NO_MATCH and not full.status[-4:-1].any()
    _same(ckpt, full, len(pairs))
    extra = len(_extra_pairs())
    for a in range(len(pairs) - extra, len(pairs)):
        w, g = R.align(*pairs[a]), _as_dict(ckpt, a)
        for k in ("status", "score", "end_row", "query_start", "ref_start", "ref_end"):
            assert g[k] == w[k], (a, k, g[k], w[k])
        assert g["ops"].tolist() == w["ops"].tolist() and g["lens"].tolist() == w["lens"].tolist(), a
    # the second extra pair does end two strips above its last strip
    a = len(pairs) - extra + 1
    assert -(-len(pairs[a][0]) // 512) - 1 - (int(ckpt.end_row[a]) - 1) // 512 == 2


def test_an_alignment_over_the_trace_budget_aligns_in_checkpointed_memory():
    """The pairs and the budget of test_gpu_duplex_align.test_statuses_leave_the_rest_of_the_batch_alone."""
    from remora_amd import duplex_utils as DU

    rng = np.random.default_rng(3)
    d = _random(rng, 700)
    s = _mutate(rng, d)
    big_d = _random(rng, 1500)
    pairs = [(s, d), (_mutate(rng, big_d), big_d), ("ACGU", "ACGT"), ("", "ACGT"), ("ACGT", ""), ("ACGT", "ACGTRACGT"), (d, s)]
    budget = DU.trace_bytes(len(s) + 200, len(d) + 200)
    rest = [DU.STATUS_BAD_BASE, DU.STATUS_EMPTY, DU.STATUS_EMPTY, DU.STATUS_BAD_BASE, DU.STATUS_OK]
    full = DU.align_batch(pairs, trace_budget=budget, mode="full")
    assert full.status.tolist() == [DU.STATUS_OK, DU.STATUS_OVER_BUDGET] + rest and full.n_checkpointed == 0
    unlimited = DU.align_batch(pairs)
    assert unlimited.status.tolist() == [DU.STATUS_OK, DU.STATUS_OK] + rest
    for mode in ("checkpoint", "auto"):
        res = DU.align_batch(pairs, trace_budget=budget, mode=mode)
        assert res.status.tolist() == [DU.STATUS_OK, DU.STATUS_OK] + rest, mode
        assert res.n_checkpointed == 3, mode
        _same(res, unlimited, len(pairs))
    maps = DU.map_simplexes_to_duplexes(pairs[:3], trace_budget=budget, mode="auto")
    assert isinstance(maps[0], DU.SimplexDuplexMapping) and isinstance(maps[1], DU.SimplexDuplexMapping) and isinstance(maps[2], str)


def test_budget_groups_give_the_same_bytes(grid):
    from remora_amd import duplex_utils as DU

    pairs, full, _ = grid
    sizes = [DU.checkpoint_bytes(len(s), len(d)) for s, d in pairs]
    small = DU.align_batch(pairs, trace_budget=2 * max(sizes), mode="checkpoint")
    assert small.n_groups >= 3 and small.n_checkpointed == len(pairs)
    _same(small, full, len(pairs))
    # a budget below one alignment's own footprint: that alignment alone is refused
    big = int(np.argmax(sizes))
    assert sizes.count(sizes[big]) == 1
    tight = DU.align_batch(pairs, trace_budget=sizes[big] - 1, mode="checkpoint")
    want = full.status.copy()
    want[big] = DU.STATUS_OVER_BUDGET
    assert tight.status.tolist() == want.tolist() and tight.n_checkpointed == len(pairs) - 1
    assert not tight.n_runs[big] and not tight.score[big]
    for a in range(len(pairs)):
        if a != big:
            assert _as_dict(tight, a)["score"] == _as_dict(full, a)["score"]
            assert tight.words[tight.run_off[a]:tight.run_off[a] + tight.n_runs[a]].tobytes() == \
                full.words[full.run_off[a]:full.run_off[a] + full.n_runs[a]].tobytes(), a


def test_auto_stores_the_trace_where_the_call_fits_at_once(grid):
    from remora_amd import duplex_utils as DU

    pairs, full, _ = grid
    auto = DU.align_batch(pairs, mode="auto")
    assert auto.n_groups == 1 and auto.n_checkpointed == 0
    _same(auto, full, len(pairs))
    tight = DU.align_batch(pairs, trace_budget=2 * max(DU.trace_bytes(len(s), len(d)) for s, d in pairs), mode="auto")
    assert tight.n_checkpointed == len(pairs)
    _same(tight, full, len(pairs))


def test_fixture_pairs_under_a_small_budget():
    from remora_amd import duplex_utils as DU

    pairs = fixture_alignments()
    long_ones = [len(d) > 10000 for _, d in pairs]
    assert sum(long_ones) == 2 and all(-(-len(s) // 512) == 48 for (s, _), big in zip(pairs, long_ones) if big)
    want = DU.align_batch(pairs)
    assert want.status.tolist() == [0, 0, 0, 0]
    got = DU.align_batch(pairs, trace_budget=64 << 20, mode="checkpoint")
    assert got.n_checkpointed == 4
    _same(got, want, len(pairs))
    full = DU.align_batch(pairs, trace_budget=64 << 20, mode="full")
    assert full.status.tolist() == [DU.STATUS_OVER_BUDGET if big else DU.STATUS_OK for big in long_ones]


def test_file_to_file_under_a_small_budget(tmp_path):
    """infer_duplex loses no pair to the budget: the record bytes are those of the default budget."""
    import torch

    from duplex_fixture import DUPLEX_BAM, PAIRS, SIMPLEX_BAM, duplex_pod5
    from oracle import oracle as O
    from remora_amd import io as rio
    from remora_amd.inference import infer_duplex
    from remora_amd.model_util import load_model
    from test_gpu_parity import _mint_pt, _real_reads_golden

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    model, md = load_model(_mint_pt(tmp_path, _real_reads_golden("can"), O), device=0)
    pod5 = duplex_pod5(tmp_path)
    raws = []
    for name, budget in (("default.bam", None), ("small.bam", 64 << 20)):
        out = str(tmp_path / name)
        errs = infer_duplex(simplex_pod5_path=pod5, simplex_bam_path=SIMPLEX_BAM, duplex_bam_path=DUPLEX_BAM, pairs_path=PAIRS, model=model,
                            model_metadata=md, out_bam=out, trace_budget=budget)
        assert errs == {}, (name, errs)
        raws.append([bytes(r.raw) for r in rio.iter_bam_records(out)])
    assert len(raws[0]) == 2 and raws[1] == raws[0]
