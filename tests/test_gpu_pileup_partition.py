"""`analyze pileup_modbams --partition-tag` on the GPU: the stamp kernel on hand-made words against numpy, and the partitioned
run against what it replaces - the input split by the tag's value on the host, one BAM per label, each piled by the
unpartitioned run.  Every comparison is between integers and bytes."""
import ctypes
import os
import re
import struct
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import modbam_restate as mr
import test_gpu_pileup as tp
import test_gpu_pileup_ref as tpr
from conftest import ROOT

pytestmark = pytest.mark.gpu

REFS, ALPHABET = tp.REFS, tp.ALPHABET
FIXED = dict(filter_threshold=0.6, pct_filt=None)
HP_FORMS = {"c": "<b", "C": "<B", "s": "<h", "i": "<i"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


# ---- 1. the stamp kernel ------------------------------------------------------------------------------------------------------
def stamp(eng, torch, words, out_off, part, shift, n_records=None, n_words=None):
    """rmr_pileup_stamp_partition on copies of the arrays -> (rc, the words afterwards)."""
    from remora_amd import _lib as L

    dev = eng.torch_device
    d_words = torch.from_numpy(np.asarray(words, np.uint64).view(np.int64).copy()).to(dev)
    d_off = torch.from_numpy(np.asarray(out_off, np.int64)).to(dev)
    d_part = torch.from_numpy(np.asarray(part, np.int32)).to(dev)
    pad = torch.zeros(1, dtype=torch.int64, device=dev)  # (an empty tensor has no address)
    rc = L.lib().rmr_pileup_stamp_partition(eng.handle, len(part) if n_records is None else n_records, d_off.data_ptr(),
                                            d_part.data_ptr() if len(part) else pad.data_ptr(), int(shift),
                                            d_words.data_ptr() if len(words) else pad.data_ptr(), len(words) if n_words is None else n_words)
    eng.synchronize()
    return rc, d_words.cpu().numpy().view(np.uint64)


def stamped(words, out_off, part, shift):
    """numpy: every word of record r gets part[r] << shift."""
    sizes = np.diff(np.asarray(out_off, np.int64))
    field = np.repeat(np.asarray(part, np.uint64), sizes) << np.uint64(shift)
    return np.asarray(words, np.uint64) | field


def _sizes(case, rng):
    if case == "one_word":
        return [1]
    if case == "empty_records":  # without words at the start, in the middle (two in a row) and at the end
        return [0, 3, 0, 0, 5, 1, 0]
    if case == "long_record":    # more words than a block has threads, between short ones
        return [2, 300, 1, 257, 256, 255]
    sizes = rng.integers(0, 40, 1000)
    sizes[rng.integers(0, 1000, 200)] = 0
    sizes[rng.integers(0, 1000, 5)] = rng.integers(256, 900, 5)
    return sizes.tolist()


@pytest.mark.parametrize("contig_bits,part_bits", [(0, 8), (16, 8), (23, 1)])  # the shifts 36 and 52, and the top one, 59
@pytest.mark.parametrize("case", ["one_word", "empty_records", "long_record", "thousand_records"])
def test_stamp_kernel_on_hand_made_words(torch_cuda, case, contig_bits, part_bits):
    from remora_amd.engine import get_engine
    from remora_amd.pileup import partition_bit_plan

    eng, rng = get_engine(None), np.random.default_rng(41)
    shift, top = 36 + contig_bits, (1 << part_bits) - 1
    assert partition_bit_plan(max(1 << contig_bits, 1), "HP")[:4] == (contig_bits, part_bits, top, shift)
    sizes = _sizes(case, rng)
    out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(out_off[-1])
    words = rng.integers(0, 1 << shift, n, dtype=np.uint64)  # site words as the emit leaves them: nothing above the contig index
    words[: n // 2] |= np.uint64((1 << shift) - 1) * (rng.integers(0, 4, n // 2) == 0).astype(np.uint64)  # every lower bit set in some
    for ids in ([0, 1, top], [top], [1], [0]):
        part = rng.choice(ids, len(sizes)).astype(np.int32)
        owners = np.nonzero(np.asarray(sizes) > 0)[0]
        part[owners[: len(ids)]] = ids[: owners.size]  # every id on a record that has words, as far as there are such records
        rc, got = stamp(eng, torch_cuda, words, out_off, part, shift)
        want = stamped(words, out_off, part, shift)
        assert rc == 0 and np.array_equal(got, want), (case, shift, ids)
        low = np.uint64((1 << shift) - 1)
        assert np.array_equal(got & low, words & low)                        # every bit below the shift is unchanged
        rec = np.repeat(np.arange(len(sizes)), sizes)
        assert np.array_equal(got[part[rec] == 0], words[part[rec] == 0])     # rows of id 0 are bit-identical
        assert np.array_equal(got >> np.uint64(shift), part[rec].astype(np.uint64))
        assert int(got.max(initial=0)) < 1 << 60
    # the words the offsets do not cover stay as they are: nothing is stored at or behind n_words
    if n > 4:
        rc, got = stamp(eng, torch_cuda, words, out_off, np.full(len(sizes), top, np.int32), shift, n_words=n - 3)
        assert rc == 0 and np.array_equal(got[n - 3 :], words[n - 3 :]) and np.array_equal(got[: n - 3], words[: n - 3] | np.uint64(top << shift))


def test_stamp_of_no_record_launches_nothing_and_bad_arguments_are_refused(torch_cuda):
    from remora_amd import _lib as L
    from remora_amd.engine import get_engine

    eng, lib = get_engine(None), L.lib()
    words, off, part = np.arange(5, dtype=np.uint64), np.array([0, 2, 5], np.int64), np.array([1, 1], np.int32)
    eng.synchronize()
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        rc, got = stamp(eng, torch_cuda, words, off, part, 36, n_records=0)
        assert rc == 0 and np.array_equal(got, words)
        for kw, text in ((dict(n_records=-1), b"n_records"), (dict(n_words=-1), b"n_records or n_words"), (dict(shift=35), b"bit 36 to 59"),
                         (dict(shift=60), b"bit 36 to 59")):
            args = dict(shift=36)
            args.update(kw)
            rc, got = stamp(eng, torch_cuda, words, off, part, **args)
            assert rc != 0 and text in lib.rmr_last_error() and np.array_equal(got, words), kw
        t = torch_cuda.zeros(8, dtype=torch_cuda.int64, device=eng.torch_device)
        for null in range(4):
            ptrs = [eng.handle, t.data_ptr(), t.data_ptr(), t.data_ptr()]
            ptrs[null] = None
            assert lib.rmr_pileup_stamp_partition(ptrs[0], 1, ptrs[1], ptrs[2], 36, ptrs[3], 0) != 0 and b"NULL" in lib.rmr_last_error()
        assert "pileup_stamp" not in eng.profile(), eng.profile()
        rc, got = stamp(eng, torch_cuda, words, off, part, 36)
        assert rc == 0 and eng.profile()["pileup_stamp"][1] == 1  # one launch, under its own name
    finally:
        eng.profile_enable(False)


# ---- 2. the synthetic input, tagged ---------------------------------------------------------------------------------------------
def hp_tag(form, value, tag=b"HP"):
    return tag + form.encode() + struct.pack(HP_FORMS[form], value)


def write_bam(path, refs, records):
    """mr.write_bam with the record's `aux` bytes behind its modified-base tags, and names of its own."""
    from remora_amd.io import BamWriter

    with BamWriter(str(path), mr.bam_header(refs), threads=1) as w:
        for rec in records:
            w.write(mr.bam_record(rec["name"], rec["flag"], rec["ref_id"], rec["pos"], rec["cigar"], rec["seq"],
                                  mr.mod_tags(rec["mm"], rec["ml"]) + rec.get("aux", b""), rec["has_md"]))


def tagged_records():
    """The records of test_gpu_pileup's synthetic input (two contigs, both strands, codes h and m, its records without MM,
    unmapped, secondary ...): one of every four untagged - another of the four each time, so that every contig and strand has
    some - the others HP 1 or 2, written as c, C, s and i in turn."""
    recs, genome = tp._synthetic()
    out, j = [], 0
    for i, rec in enumerate(recs):
        rec = dict(rec, name=f"read{i}", label="ungrouped")
        if i % 4 != (i // 4) % 4:
            value = 1 + (j // 2 + j // 7) % 2
            rec["aux"], rec["label"] = hp_tag("cCsi"[j % 4], value), str(value)
            j += 1
        out.append(rec)
    return out, genome


def same_rows(got, want):
    for f in ("ref_id", "pos", "strand", "counts"):
        assert getattr(got, f).dtype == getattr(want, f).dtype and np.array_equal(getattr(got, f), getattr(want, f)), f
    assert got.n_calls == want.n_calls and got.threshold_k == want.threshold_k and got.combined == want.combined
    assert got.partition is None and got.partition_labels is None and got.ref_names == want.ref_names and got.alphabet == want.alphabet


def same_partitioned(a, b):
    for f in ("ref_id", "pos", "strand", "counts", "partition"):
        assert getattr(a, f).dtype == getattr(b, f).dtype and getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert a.partition_labels == b.partition_labels and a.n_calls == b.n_calls and a.threshold_k == b.threshold_k and a.partition_tag == b.partition_tag


def site_sums(tables):
    out = {}
    for t in tables:
        for key, row in zip(zip(t.ref_id.tolist(), t.pos.tolist(), t.strand.tolist()), t.counts.tolist()):
            out[key] = [a + b for a, b in zip(out.get(key, [0] * len(row)), row)]
    return out


@pytest.fixture(scope="module")
def hp(tmp_path_factory, torch_cuda):
    """The tagged input, one BAM per label, and the runs the tests share: the partitioned one at a fixed threshold and, per
    label, today's run on that label's BAM."""
    from remora_amd.pileup import partition_tables, pileup_modbams

    recs, genome = tagged_records()
    d = tmp_path_factory.mktemp("pileup_partition")
    path = str(d / "tagged.bam")
    write_bam(path, REFS, recs)
    by_label = {}
    for label in ("1", "2", "ungrouped"):
        by_label[label] = str(d / f"only_{label}.bam")
        write_bam(by_label[label], REFS, [r for r in recs if r["label"] == label])
    table = pileup_modbams(path, ALPHABET, partition_tag="HP", **FIXED)
    alone = {label: pileup_modbams(p, ALPHABET, **FIXED) for label, p in by_label.items()}
    return dict(recs=recs, genome=genome, dir=d, path=path, by_label=by_label, table=table, subs=partition_tables(table), alone=alone)


def test_tagged_input_is_what_the_issue_asks_for(hp):
    recs = hp["recs"]
    assert 55 <= len(recs) <= 70 and {r["ref_id"] for r in recs} >= {0, 1} and {r["flag"] & 16 for r in recs} == {0, 16}
    forms = {r["aux"][2:3] for r in recs if "aux" in r}
    assert forms == {b"c", b"C", b"s", b"i"} and {r["label"] for r in recs} == {"1", "2", "ungrouped"}
    assert abs(sum(r["label"] == "ungrouped" for r in recs) - len(recs) / 4) <= 1
    for label in ("1", "2", "ungrouped"):  # both contigs and both strands in every partition
        assert {(r["ref_id"], r["flag"] & 16) for r in recs if r["label"] == label and r["mm"]} >= {(0, 0), (0, 16), (1, 0), (1, 16)}, label
    assert any(r["mm"] is None for r in recs) and sum(bool(r["flag"] & 4) for r in recs) == 1 and sum(bool(r["flag"] & 0x100) for r in recs) == 1
    assert any("h" in (r["mm"] or "") and "m" in (r["mm"] or "") for r in recs)


def test_each_label_equals_the_run_on_that_labels_records(hp, tmp_path):
    from remora_amd.pileup import pileup_modbams, write_partitioned

    table, subs, alone = hp["table"], hp["subs"], hp["alone"]
    assert table.partition_labels == ["1", "2", "ungrouped"] and list(subs) == table.partition_labels and table.partition_tag == "HP"
    assert table.partition.dtype == np.int32 and table.partition.size == table.pos.size and table.hist is None
    keys = list(zip(table.partition.tolist(), table.ref_id.tolist(), table.pos.tolist(), table.strand.tolist()))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)  # rows by (label order, ref_id, pos, strand)
    assert int(table.ref_id.max()) == 1 and table.n_calls == sum(t.n_calls for t in alone.values()) == int(table.counts.sum())
    rows = write_partitioned(table, tmp_path / "p.bed", tmp_path / "p.tsv", min_coverage=2)
    for label, name in (("1", "HP_1"), ("2", "HP_2"), ("ungrouped", "ungrouped")):
        same_rows(subs[label], alone[label])
        want_bed, want_tsv = tp.files_of(alone[label], tmp_path, f"alone_{name}", min_coverage=2)
        assert tp.files_of(subs[label], tmp_path, f"sub_{name}", min_coverage=2) == (want_bed, want_tsv)
        assert (tmp_path / f"p.{name}.bed").read_text() == want_bed and (tmp_path / f"p.{name}.tsv").read_text() == want_tsv
        assert rows[label] == want_bed.count("\n") > 0
    # the per-site sum over the labels is the unpartitioned run on the whole file
    whole = pileup_modbams(hp["path"], ALPHABET, **FIXED)
    assert whole.partition is None and whole.partition_labels is None and whole.partition_tag is None
    sums = site_sums(subs.values())
    assert sorted(sums) == list(zip(whole.ref_id.tolist(), whole.pos.tolist(), whole.strand.tolist()))
    assert [sums[k] for k in sorted(sums)] == whole.counts.tolist() and whole.n_calls == table.n_calls
    # not vacuous: three labels with rows, sites shared between labels and sites of one label alone
    sites = {label: set(zip(t.ref_id.tolist(), t.pos.tolist(), t.strand.tolist())) for label, t in subs.items()}
    assert all(len(s) > 100 for s in sites.values())
    assert len(sites["1"] & sites["2"]) > 20 and len(sites["1"] - sites["2"] - sites["ungrouped"]) > 20 and len(sites["ungrouped"] - sites["1"] - sites["2"]) > 0


def test_one_threshold_for_the_whole_input(hp, tmp_path):
    from remora_amd.pileup import partition_tables, pileup_modbams

    whole = pileup_modbams(hp["path"], ALPHABET, pct_filt=10)
    table = pileup_modbams(hp["path"], ALPHABET, pct_filt=10, partition_tag="HP")
    assert table.threshold_k == whole.threshold_k and table.hist.dtype == np.int64 and np.array_equal(table.hist, whole.hist)
    assert 0 < table.threshold_k < 512 and table.n_calls == whole.n_calls == int(whole.hist.sum())
    for label, sub in partition_tables(table).items():
        want = pileup_modbams(hp["by_label"][label], ALPHABET, filter_threshold=Fraction(table.threshold_k, 512), pct_filt=None)
        assert sub.threshold_k == table.threshold_k and sub.hist is table.hist
        same_rows(sub, want)
        assert tp.files_of(sub, tmp_path, f"sub_{label}") == tp.files_of(want, tmp_path, f"want_{label}")


def test_buffer_batch_and_file_split_do_not_matter(hp, tmp_path):
    from remora_amd.pileup import pileup_modbams, write_partitioned

    table, recs = hp["table"], hp["recs"]
    assert table.n_flushes == 1
    same_partitioned(pileup_modbams(hp["path"], ALPHABET, partition_tag="HP", batch=1, **FIXED), table)
    same_partitioned(pileup_modbams(hp["path"], ALPHABET, partition_tag="HP", batch=7, **FIXED), table)
    got = pileup_modbams(hp["path"], ALPHABET, partition_tag="HP", buffer_calls=64, **FIXED)
    assert got.n_flushes == -(-got.n_calls // 64) > 1
    same_partitioned(got, table)
    # two files, in either order: the ids are given in another order, the table is the same
    p1, p2 = str(tmp_path / "half1.bam"), str(tmp_path / "half2.bam")
    write_bam(p1, REFS, recs[:25])
    write_bam(p2, REFS, recs[25:])
    first = [next(r["label"] for r in half if "aux" in r) for half in (recs[:25], recs[25:])]
    assert first[0] != first[1]  # the first value seen, id 1, differs between the orders
    want = write_partitioned(table, tmp_path / "whole.bed", tmp_path / "whole.tsv")
    for tag, order in (("ab", [p1, p2]), ("ba", [p2, p1])):
        got = pileup_modbams(order, ALPHABET, partition_tag="HP", **FIXED)
        same_partitioned(got, table)
        assert write_partitioned(got, tmp_path / f"{tag}.bed", tmp_path / f"{tag}.tsv") == want
        for name in ("HP_1", "HP_2", "ungrouped"):
            for ext in ("bed", "tsv"):
                assert (tmp_path / f"{tag}.{name}.{ext}").read_bytes() == (tmp_path / f"whole.{name}.{ext}").read_bytes()
    # a buffer of one call, a flush per call, on a smaller input: a site's calls of one partition straddle many flushes
    small = str(tmp_path / "small.bam")
    write_bam(small, REFS, recs[:8] + recs[44:52])
    a = pileup_modbams(small, ALPHABET, partition_tag="HP", **FIXED)
    assert a.n_flushes == 1 and a.partition_labels == ["1", "2", "ungrouped"] and a.counts.sum(axis=1).max() >= 2
    one = pileup_modbams(small, ALPHABET, partition_tag="HP", buffer_calls=1, **FIXED)
    assert one.n_flushes == one.n_calls > 1
    same_partitioned(one, a)


def test_with_a_reference_and_with_a_region(hp, tmp_path):
    from remora_amd.pileup import RefGenome, partition_tables, pileup_modbams

    fasta = tmp_path / "genome.fa"
    fasta.write_text(tpr.fasta_text([(name, seq) for (name, _), seq in zip(REFS, hp["genome"])], 60))
    with RefGenome.from_fasta(fasta, [r[0] for r in REFS], [r[1] for r in REFS]) as genome:
        for tag, kw in (("cpg", dict(ref=genome, motifs=[("CG", 0)], combine_strands=True)), ("region", dict(region="ctgB:400-1500")),
                        ("cpg_region", dict(ref=genome, motifs=[("CG", 0)], combine_strands=True, region="ctgA:0-1200"))):
            table = pileup_modbams(hp["path"], ALPHABET, partition_tag="HP", **FIXED, **kw)
            assert table.partition_labels == ["1", "2", "ungrouped"] and table.combined == ("ref" in kw)
            if "region" in kw:
                rid, lo, hi = (1, 400, 1500) if tag == "region" else (0, 0, 1200)
                assert set(table.ref_id.tolist()) == {rid} and lo <= int(table.pos.min()) and int(table.pos.max()) < hi
            if "ref" in kw:
                assert not table.strand.any() and all(hp["genome"][r][p : p + 2] == "CG" for r, p in zip(table.ref_id.tolist(), table.pos.tolist()))
            for label, sub in partition_tables(table).items():
                want = pileup_modbams(hp["by_label"][label], ALPHABET, **FIXED, **kw)
                assert want.pos.size > 5
                same_rows(sub, want)
                assert tp.files_of(sub, tmp_path, f"{tag}_sub_{label}") == tp.files_of(want, tmp_path, f"{tag}_want_{label}")


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def _short(i, aux):
    return dict(name=f"short{i}", seq="ACGTC", flag=0, ref_id=0, pos=10 + i % 50, cigar=[("M", 5)], mm="C+m?,0;", ml=[200], has_md=True, aux=aux)


def test_refusals_launch_nothing_and_leave_no_file(torch_cuda, tmp_path, capsys):
    """The inputs are of one batch: what a partition tag is refused for is found when the batch is read, before the batch's
    first launch."""
    from remora_amd.__main__ import main
    from remora_amd.engine import get_engine

    one_contig = [("ctgA", 2000)]
    inputs = {
        "values": (one_contig, [_short(i, hp_tag("i", 1000 + i)) for i in range(256)],
                   r"--partition-tag HP: more than 255 distinct values - HP = '1255' of read short255"),
        "fits": (one_contig, [_short(i, hp_tag("i", 1000 + i)) for i in range(255)], None),
        "z_typed": (REFS, [_short(0, hp_tag("c", 1)), _short(1, b"HPZ1\x00")], "read short1 of .* has HP of type Z"),
        "mixed": (REFS, [_short(0, hp_tag("c", 1)), _short(1, b"HPA1")], "HP is a character in read short1 of .* and an integer in the records before"),
    }
    eng = get_engine(None)
    eng.synchronize()
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        for name, (refs, recs, message) in inputs.items():
            if message is None:
                continue
            path = str(tmp_path / f"{name}.bam")
            write_bam(path, refs, recs)
            for threshold in (["--filter-threshold", "0.5"], ["--pct-filt", "10"]):
                rc = main(["analyze", "pileup_modbams", "--bam", path, "--canonical-base", "C", "--mod-bases", "m", "--out-bed", str(tmp_path / f"{name}.bed"),
                           "--counts-filename", str(tmp_path / f"{name}.tsv"), "--partition-tag", "HP"] + threshold)
                assert rc == 1 and re.search(message, capsys.readouterr().err), name
        assert not any(k.startswith(("pileup_", "modbam_")) for k in eng.profile()), eng.profile()
        assert sorted(f for f in os.listdir(tmp_path) if not f.endswith(".bam")) == []
    finally:
        eng.profile_enable(False)
    # 255 values fit: a partition each
    from remora_amd.pileup import pileup_modbams

    refs, recs, _ = inputs["fits"]
    path = str(tmp_path / "fits.bam")
    write_bam(path, refs, recs)
    got = pileup_modbams(path, ["C", "m"], partition_tag="HP", **FIXED)
    assert got.partition_labels == [str(1000 + i) for i in range(255)] and got.partition.tolist() == sorted(got.partition.tolist())
    assert got.n_calls == 255 and np.array_equal(np.bincount(got.partition), np.ones(255, np.int64)) and got.counts[:, 1].sum() == 255


# ---- 4. the command line --------------------------------------------------------------------------------------------------------
def test_command_line_writes_the_api_bytes(hp, tmp_path):
    from remora_amd.pileup import pileup_modbams, write_partitioned

    plain = str(tmp_path / "untagged.bam")
    write_bam(plain, REFS, [{k: v for k, v in r.items() if k != "aux"} for r in hp["recs"]])
    base = [sys.executable, "-m", "remora_amd", "analyze", "pileup_modbams", "--canonical-base", "C", "--mod-bases", "h", "m", "--filter-threshold", "0.6"]
    runs = {"tagged": ["--bam", hp["path"], "--partition-tag", "HP"], "untagged": ["--bam", plain, "--partition-tag", "HP"], "without": ["--bam", plain]}
    procs = {t: subprocess.Popen(base + extra + ["--out-bed", str(tmp_path / f"{t}.bed"), "--counts-filename", str(tmp_path / f"{t}.tsv")],
                                 cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for t, extra in runs.items()}
    errs = {}
    for t, p in procs.items():
        _, errs[t] = p.communicate(timeout=300)
        assert p.returncode == 0, errs[t]
    written = sorted(f for f in os.listdir(tmp_path) if f.endswith((".bed", ".tsv")))
    assert written == sorted([f"tagged.{n}.{e}" for n in ("HP_1", "HP_2", "ungrouped") for e in ("bed", "tsv")] +
                             ["untagged.ungrouped.bed", "untagged.ungrouped.tsv", "without.bed", "without.tsv"])
    rows = write_partitioned(hp["table"], tmp_path / "api.bed", tmp_path / "api.tsv")
    for name in ("HP_1", "HP_2", "ungrouped"):
        for ext in ("bed", "tsv"):
            assert (tmp_path / f"tagged.{name}.{ext}").read_bytes() == (tmp_path / f"api.{name}.{ext}").read_bytes()
    assert "bedMethyl rows per HP: " + ", ".join(f"{label}: {n}" for label, n in rows.items()) in errs["tagged"]
    # without the argument: the parent's bytes; an input without the tag: one partition, the same bytes again
    read = lambda t: ((tmp_path / f"{t}.bed").read_text(), (tmp_path / f"{t}.tsv").read_text())  # noqa: E731
    assert read("without") == tp.files_of(pileup_modbams(plain, ALPHABET, **FIXED), tmp_path, "api_plain")
    assert read("untagged.ungrouped") == read("without")
