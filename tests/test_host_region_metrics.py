"""CPU-only checks of the region API (remora_amd/region_metrics.py, io.RefRegion, io.Read.extract_basecall_region): the pair
plan against a brute-force restatement, the region helpers, and the sequence functions against the reference's values
(tests/golden/region_metrics.npz, written by tools/gen_golden.py --only regions)."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden

DATA = os.path.join(GOLDEN, "data")


@pytest.fixture(scope="module")
def fx():
    return golden("region_metrics.npz")


def _region(fx, name):
    from remora_amd import io as rio

    ctg, strand, start, end = fx["regions"][list(fx["region_names"]).index(name)]
    return rio.RefRegion(str(ctg), str(strand), int(start), int(end))


@pytest.fixture(scope="module")
def can_records():
    from remora_amd import io as rio

    return list(rio.iter_bam_records(os.path.join(DATA, "can_mappings.bam"), want_ref=True))


def _covering(records, reg):
    """get_reg_bam_reads restated (src/remora/io.py:540-549) on parsed records, file order."""
    from remora_amd import io as rio

    return [r for r in records if not r.is_unmapped and r.reference_name == reg.ctg and r.reference_start < reg.end
            and r.reference_end > reg.start and rio.read_is_primary(r) and rio.strands_match(reg.strand, r)]


def test_pair_plan_against_a_brute_force_restatement():
    """plan_region_pairs over random spans and regions against the reference's arithmetic written out per read
    (compute_per_base_metric :2438-2460, extract_ref_reg :2359-2366, get_reg_bam_reads :540-549)."""
    from remora_amd import io as rio

    rng = np.random.default_rng(3)
    names = ["c0", "c1", "c2"]
    n = 400
    ref_id = rng.integers(-1, 3, size=n)
    start = rng.integers(0, 300, size=n)
    length = rng.integers(0, 120, size=n)
    flag = rng.choice([0, 16, 4, 256, 272, 2048, 2064], size=n, p=[0.4, 0.4, 0.04, 0.04, 0.04, 0.04, 0.04])
    regions = []
    for _ in range(40):
        s = int(rng.integers(0, 380))
        regions.append(rio.RefRegion(names[int(rng.integers(0, 3))], [None, "+", "-"][int(rng.integers(0, 3))], s, s + int(rng.integers(1, 90))))
    regions.append(rio.RefRegion("c1", "+", 77))  # end=None: one position
    regions.append(rio.RefRegion("elsewhere", "+", 0, 1000))
    for extract in (False, True):
        for ref_orient in (True, False):
            got = rio.plan_region_pairs(regions, names, ref_id, start, length, flag, ref_orient=ref_orient, extract=extract)
            want = []
            for r, reg in enumerate(regions):
                end = reg.start + 1 if reg.end is None else reg.end
                row = 0
                for i in range(n):
                    rev = bool(flag[i] & 16)
                    if flag[i] & (4 | 256 | 2048) or ref_id[i] < 0 or length[i] == 0 or names[ref_id[i]] != reg.ctg:
                        continue
                    if reg.strand is not None and rev != (reg.strand == "-"):
                        continue
                    r_end = start[i] + length[i]
                    if not (start[i] < end and r_end > reg.start):
                        continue
                    st, en = (r_end - end, r_end - reg.start) if rev else (reg.start - start[i], end - start[i])
                    if extract:
                        first, last, lead, flip = max(0, st), min(en, length[i]), 0, rev
                    else:
                        lead = -st if st < 0 else 0
                        first, last, flip = max(st, 0), min(en, length[i]), rev and ref_orient
                    want.append((r, i, first, last, lead, row, end - reg.start, int(flip)))
                    row += 1
            want = np.asarray(want, np.int64).reshape(-1, 8)
            cols = np.stack([got[k] for k in ("region", "read", "first", "last", "lead", "row", "rlen", "flip")], axis=1)
            assert np.array_equal(cols, want), (extract, ref_orient)
            assert want.shape[0] > 200
            # what the kernels' wrapper insists on holds for every planned pair
            assert (want[:, 2] < want[:, 3]).all() and (want[:, 4] + want[:, 3] - want[:, 2] <= want[:, 6]).all()


def test_ref_region_helpers():
    from remora_amd import RemoraError
    from remora_amd import io as rio

    assert rio.RefRegion("c", "+", 5).len == 1 and rio.RefRegion("c", "+", 5, 9).len == 4
    reg = rio.RefRegion.parse_ref_region_str("chr13:52310001-52310100:-")
    assert (reg.ctg, reg.strand, reg.start, reg.end) == ("chr13", "-", 52310000, 52310100)
    assert rio.RefRegion.parse_ref_region_str("a:b:3-9", req_strand=False) == rio.RefRegion("a:b", None, 2, 9)
    assert rio.RefRegion.parse_ref_region_str("c:3-9:+", req_strand=False).strand == "+"
    for bad, msg in (("c:3-9", "Invalid reference region: c:3-9"), ("c:0-9:+", "Invalid reference start coordinate")):
        with pytest.raises(RemoraError, match=re.escape(msg)):
            rio.RefRegion.parse_ref_region_str(bad)
    fwd, rev = rio.RefRegion("c", "+", 10, 20), rio.RefRegion("c", "-", 10, 20)
    assert fwd.adjust(-2, 3) == rio.RefRegion("c", "+", 8, 23) and rev.adjust(-2, 3) == rio.RefRegion("c", "-", 8, 23)
    assert fwd.adjust(-2, 3, ref_orient=False) == rio.RefRegion("c", "+", 8, 23)
    assert rev.adjust(-2, 3, ref_orient=False) == rio.RefRegion("c", "-", 7, 22)
    assert rio.RefRegion("c", "-", 10).adjust(-2, 3, ref_orient=False) == rio.RefRegion("c", "-", 7, None)
    assert list(rio.parse_bed_lines(os.path.join(DATA, "ref_regions.bed")))  # the reference's own region file parses


def test_compute_base_space_sig_coords_and_ref_sig_coords(fx):
    from remora_amd import io as rio

    m = np.asarray([0, 2, 2, 6, 7], np.int64)
    want = np.asarray([0, 0.5, 2, 2.25, 2.5, 2.75, 3.0])  # a sample's share of the way through its base; an empty base is passed over
    assert np.array_equal(rio.compute_base_space_sig_coords(m), want)
    assert np.array_equal(rio.compute_base_space_sig_coords(m + 40), np.interp(np.arange(7), m + 40, np.arange(5)))
    for name in ("a_fwd", "a_rev", "b_rev"):
        k = f"x_{name}_r0"
        ctg, strand, start, end = fx[f"{k}_ref_reg"]
        rr = rio.ReadRefReg(str(fx[f"{k}_read_id"]), fx[f"{k}_sig"], str(fx[f"{k}_seq"]), fx[f"{k}_map"],
                            rio.RefRegion(str(ctg), str(strand), int(start), int(end)), int(fx[f"{k}_sig_start"]))
        assert np.array_equal(rr.ref_sig_coords, fx[f"{k}_coords"]), name


def test_sequences_from_reads_against_the_reference(fx, can_records):
    """get_ref_int_seq_from_reads / get_ref_seq_from_reads / get_ref_seq_and_levels_from_reads on the records that cover the
    golden's regions.  Levels are compared where the whole k-mer is covered ACGT (everywhere in these regions: asserted when the
    golden was written); on the reverse strand the golden holds only the integer form (tools/gen_golden.py says why)."""
    from remora_amd import io as rio
    from remora_amd.refine_signal_map import SigMapRefiner

    refiner = SigMapRefiner(kmer_model_filename=os.path.join(DATA, "levels_4mer.txt"), do_rough_rescale=True, scale_iters=0, do_fix_guage=True)
    assert [refiner.bases_before, refiner.bases_after] == fx["levels_context"].tolist()
    for name in ("a_fwd", "a_rev", "b_fwd", "b_rev"):
        reg = _region(fx, name)
        recs = _covering(can_records, reg)
        assert [r.query_name for r in recs] == fx[f"m_{name}_can_dwell_mean_sd_ref_s0_ids"].tolist()
        for orient in (True, False):
            k = f"q_{name}_{'ref' if orient else 'read'}"
            ints = rio.get_ref_int_seq_from_reads(reg, recs, ref_orient=orient)
            assert ints.dtype == np.int32 and ints.min() >= 0
            assert np.array_equal(ints, fx[f"{k}_int_seq"].astype(np.int64)), k
            seq, levels = rio.get_ref_seq_and_levels_from_reads(reg, recs, refiner, ref_orient=orient)
            assert seq == rio.get_ref_seq_from_reads(reg, recs, ref_orient=orient)
            assert len(seq) == reg.len and levels.shape == (reg.len,) and np.isfinite(levels).all()
            if name.endswith("_fwd"):
                assert seq == str(fx[f"{k}_seq"]) == str(fx[f"{k}_lv_seq"]) == str(fx[f"{k}_seq_only"]), k
                assert rio.get_ref_seq_and_levels_from_reads(reg, recs, None, ref_orient=orient) == (seq, None)
                assert np.array_equal(levels, fx[f"{k}_levels"]), k
            else:  # the same bases, complemented (and reversed when read-oriented), looked up in the same table
                fwd_reg = rio.RefRegion(reg.ctg, "+", reg.start, reg.end)
                fwd = rio.get_ref_seq_from_reads(fwd_reg, recs)
                assert seq == (fwd.translate(str.maketrans("ACGT", "TGCA")) if orient else rio.revcomp(fwd))
                ctx = rio.get_ref_int_seq_from_reads(reg.adjust(-refiner.bases_before, refiner.bases_after, ref_orient=False), recs, ref_orient=False)
                want = refiner.extract_levels(ctx)[refiner.bases_before : refiner.bases_before + reg.len]
                assert np.array_equal(levels, want[::-1] if orient else want)


def test_positions_without_a_whole_kmer_get_nan(fx, can_records):
    """The stated difference: where the reference indexes its table with a k-mer that holds an uncovered (-2) or non-ACGT (-1)
    base, the level is NaN here; covered positions keep their level and uncovered bases read N."""
    from remora_amd import io as rio
    from remora_amd.refine_signal_map import SigMapRefiner

    refiner = SigMapRefiner(kmer_model_filename=os.path.join(DATA, "levels_4mer.txt"), do_rough_rescale=True, scale_iters=0, do_fix_guage=True)
    kb, ka = refiner.bases_before, refiner.bases_after
    reg = _region(fx, "b_fwd")
    late = [r for r in _covering(can_records, reg) if r.reference_start > reg.start]  # reads that begin inside the region
    assert late
    gap = min(r.reference_start for r in late) - reg.start
    seq, levels = rio.get_ref_seq_and_levels_from_reads(reg, late, refiner)
    whole, _ = rio.get_ref_seq_and_levels_from_reads(reg, _covering(can_records, reg), refiner)
    ints = rio.get_ref_int_seq_from_reads(reg, late)
    assert (ints[:gap] == -2).all() and (ints[gap:] >= 0).all()
    assert seq[:gap] == "N" * gap and seq[gap:] == whole[gap:]
    assert np.isnan(levels[: gap + kb]).all() and np.isfinite(levels[gap + kb : reg.len - ka]).all()
    assert np.array_equal(levels[gap + kb : reg.len - ka], fx["q_b_fwd_ref_levels"][gap + kb : reg.len - ka])


def test_reverse_strand_keeps_uncovered_and_n_apart(fx, can_records):
    """get_ref_int_seq_from_reads on a `-` region whose first positions nobody covers, and with an N in a record's reference
    bases: -2 where no read covers, -1 for the N, the complement elsewhere - at the mirrored places when read-oriented."""
    from remora_amd import io as rio

    reg = _region(fx, "b_rev")
    late = [r for r in _covering(can_records, _region(fx, "b_fwd")) if r.reference_start > reg.start]  # they begin inside the region
    gap = min(r.reference_start for r in late) - reg.start
    assert late and 0 < gap < reg.len - 3
    n_at = gap + 2  # an N at this position of the region, in the reference bases of every record that covers it

    class WithN:
        def __init__(self, rec):
            self.reference_start, self.reference_end = rec.reference_start, rec.reference_end
            seq = rec.get_reference_sequence()
            at = reg.start + n_at - rec.reference_start
            self._seq = seq[:at] + "N" + seq[at + 1 :] if 0 <= at < len(seq) else seq

        def get_reference_sequence(self):
            return self._seq

    recs = [WithN(r) for r in late]
    fwd = rio.get_ref_int_seq_from_reads(rio.RefRegion(reg.ctg, "+", reg.start, reg.end), recs)
    assert (fwd[:gap] == -2).all() and fwd[n_at] == -1 and (np.delete(fwd[gap:], n_at - gap) >= 0).all()
    want = np.where(fwd >= 0, 3 - fwd, fwd)
    ref_or = rio.get_ref_int_seq_from_reads(reg, recs, ref_orient=True)
    read_or = rio.get_ref_int_seq_from_reads(reg, recs, ref_orient=False)
    assert ref_or.dtype == read_or.dtype == np.int32
    assert np.array_equal(ref_or, want) and np.array_equal(read_or, want[::-1])
    assert (ref_or[:gap] == -2).all() and ref_or[n_at] == -1
    assert (read_or[reg.len - gap :] == -2).all() and read_or[reg.len - 1 - n_at] == -1
    seq = rio.get_ref_seq_from_reads(reg, recs, ref_orient=True)
    assert seq[:gap] == "N" * gap and seq[n_at] == "N" and "N" not in seq[gap:n_at] + seq[n_at + 1 :]


def test_extract_basecall_region():
    """Read.extract_basecall_region (src/remora/io.py:2310-2340) on a read put together by hand."""
    from remora_amd import RemoraError
    from remora_amd import io as rio

    dacs = np.arange(100, 140, dtype=np.int16)
    q2s = np.asarray([3, 5, 9, 9, 14, 20, 31], np.int64)
    read = rio.Read(read_id="r", dacs=dacs, seq="ACGTAC", query_to_signal=q2s, shift_dacs_to_norm=110.0, scale_dacs_to_norm=4.0,
                    shift_dacs_to_pa=2.0, scale_dacs_to_pa=0.5)
    got = read.extract_basecall_region(1, 4)
    assert isinstance(got, rio.ReadBasecallRegion) and (got.read_id, got.seq, got.start, int(got.sig_start)) == ("r", "CGT", 1, 5)
    assert np.array_equal(got.seq_to_sig_map, [0, 4, 4, 9]) and np.array_equal(got.norm_signal, (dacs[5:14] - 110.0) / 4.0)
    whole = read.extract_basecall_region()
    assert whole.seq == "ACGTAC" and np.array_equal(whole.seq_to_sig_map, q2s - 3) and whole.norm_signal.size == 28
    assert np.array_equal(read.extract_basecall_region(2, 5, signal_type="dac").norm_signal, dacs[9:20])
    assert np.array_equal(read.extract_basecall_region(2, 5, signal_type="pa").norm_signal, (dacs[9:20] - 2.0) / 0.5)
    assert q2s[0] == 3  # the read's own mapping is not re-based
    with pytest.raises(RemoraError, match="Missing query_to_signal"):
        rio.Read(read_id="r", dacs=dacs, seq="ACGT").extract_basecall_region()


def test_bam_record_reference_end(can_records):
    for rec in can_records[:6]:
        assert rec.reference_end == rec.reference_start + len(rec.get_reference_sequence())
        assert rec.is_forward != rec.is_reverse


def test_new_symbols_are_exported_and_declared():
    from remora_amd import _lib

    header = open(os.path.join(ROOT, "include", "remora_hip.h")).read()
    built = _lib.lib() if os.path.exists(_lib.LIB_PATH) else None  # (refuses a library that lacks a declared symbol)
    for name in ("rmr_region_base_metrics", "rmr_region_signals"):
        assert name in _lib.SIGNATURES and re.search(rf"\bint {name}\(", header), name
        if built is not None:
            assert hasattr(built, name), name
    names = open(os.path.join(ROOT, "remora_amd", "csrc", "engine.hip")).read()
    assert '"region_metrics", "region_signals"' in names
