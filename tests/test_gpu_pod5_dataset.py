"""A run's directory of POD5 files as the POD5 argument (io.open_pod5 -> io.Pod5Dataset, the read ids an index on the GPU:
rmr_read_index_*, csrc/k_read_index.hip) where the reference opens pod5.DatasetReader (src/remora/io.py:427,
src/remora/inference.py:481, src/remora/prepare_train_data.py:153, src/remora/parsers.py:2109).  The two fixtures
can_reads.pod5 / mod_reads.pod5 (14 reads each, no id in common; the BAMs share their reference table) make a directory; what
comes out of it - ingest batches, reads, `infer` output, a prepared dataset, k-mer levels - is what the single file gives, to the
bit."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DATA = os.path.join(HERE, "golden", "data")
POD5 = {p: os.path.join(DATA, f"{p}_reads.pod5") for p in ("can", "mod")}
BAM = {p: os.path.join(DATA, f"{p}_mappings.bam") for p in ("can", "mod")}


@pytest.fixture()
def run_dir(tmp_path):
    """Half copied, half linked: both are files of the directory."""
    import shutil

    d = tmp_path / "run"
    d.mkdir()
    shutil.copy(POD5["can"], d / "a_can.pod5")
    os.symlink(POD5["mod"], d / "b_mod.pod5")
    shutil.copy(os.path.join(DATA, "duplex_reads.pod5.part00"), d / "duplex_reads.pod5.part00")  # not a *.pod5: never opened
    return str(d)


def _batch_arrays(ib):
    """Every array of an IngestBatch, by name (device arrays copied back)."""
    out = {"keep": ib.keep, "good": ib.good, "seq": np.frombuffer(ib.seq, np.uint8), "seq_off": ib.seq_off, "iseq": ib.iseq}
    for name in ("ref_fwd_off", "map0", "cal_off", "cal_scale"):
        v = getattr(ib, name)
        if v is not None:
            out[name] = np.asarray(v)
    if ib.ref_fwd is not None:
        out["ref_fwd"] = np.frombuffer(ib.ref_fwd, np.uint8)
    if ib.dr is not None:
        dr = ib.dr
        for name in ("dacs", "s2s", "iseq", "shift", "scale", "d_sig_off", "d_seq_off"):
            out["dr." + name] = getattr(dr, name).cpu().numpy()
        out["dr.sig_off"], out["dr.seq_off"] = np.asarray(dr.sig_off), np.asarray(dr.seq_off)
        out["stub.shift"] = np.asarray([r.shift for r in ib.reads])
        out["stub.scale"] = np.asarray([r.scale for r in ib.reads])
    return out


def _ingest(pod5, bam, batch, ref_anchored, pa_scaling=None):
    from remora_amd import io as rio

    got = []
    for ib in rio.iter_ingest_batches(pod5, bam, pa_scaling=pa_scaling, batch=batch, ref_anchored=ref_anchored):
        assert isinstance(ib, rio.IngestBatch)
        got.append((list(ib.err), _batch_arrays(ib)))
    return got


def _assert_same_batches(got, want):
    assert len(got) == len(want) and len(want) > 0
    for (g_err, g), (w_err, w) in zip(got, want):
        assert g_err == w_err  # the same reasons, the same texts, the same order
        assert sorted(g) == sorted(w)
        for name in w:
            assert g[name].dtype == w[name].dtype and g[name].shape == w[name].shape, name
            assert g[name].tobytes() == w[name].tobytes(), name


@pytest.mark.parametrize("batch", [4, 5])
@pytest.mark.parametrize("ref_anchored", [False, True])
@pytest.mark.parametrize("prefix", ["can", "mod"])
def test_ingest_batches_over_the_directory_equal_the_single_file(prefix, ref_anchored, batch, run_dir, tmp_path):
    """The clean BAM and the one with records that have to be turned away (tests/test_gpu_ingest.py: a secondary alignment, an
    unmapped reverse record, a missing move table, a read the POD5 does not hold - its name is no id at all -, a trim that
    leaves too little signal, one read twice in a batch)."""
    import torch

    from test_gpu_ingest import _dirty_bam

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dirty = str(tmp_path / "dirty.bam")
    _dirty_bam(dirty, prefix, with_missing_moves=not ref_anchored)
    for bam, pa_scaling in ((BAM[prefix], None), (dirty, None), (dirty, (87.5, 14.25))):
        want = _ingest(POD5[prefix], bam, batch, ref_anchored, pa_scaling)
        _assert_same_batches(_ingest(run_dir, bam, batch, ref_anchored, pa_scaling), want)
        if bam is dirty:
            assert sum(e is not None for errs, _ in want for e in errs) == (2 if ref_anchored else 3)


def _read_fields(read):
    out = {}
    for name in ("dacs", "query_to_signal", "ref_to_signal", "mv_table"):
        v = getattr(read, name)
        out[name] = None if v is None else np.asarray(v).tobytes()
    for name in ("read_id", "seq", "ref_seq", "stride", "shift_dacs_to_pa", "scale_dacs_to_pa", "shift_pa_to_norm", "scale_pa_to_norm",
                 "shift_dacs_to_norm", "scale_dacs_to_norm", "cigar"):
        out[name] = getattr(read, name)
    out["ref_reg"] = None if read.ref_reg is None else (read.ref_reg.ctg, read.ref_reg.strand, read.ref_reg.start, read.ref_reg.end)
    out["record"] = None if read.record is None else bytes(read.record.raw)
    return out


@pytest.mark.parametrize("decode_batch", [4, 5])
@pytest.mark.parametrize("ref_anchored", [False, True])
@pytest.mark.parametrize("prefix", ["can", "mod"])
def test_reads_over_the_directory_equal_the_single_file(prefix, ref_anchored, decode_batch, run_dir, tmp_path):
    import torch

    from remora_amd import io as rio
    from test_gpu_ingest import _dirty_bam

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    dirty = str(tmp_path / "dirty.bam")
    _dirty_bam(dirty, prefix)
    for bam in (BAM[prefix], dirty):
        runs = []
        for pod5 in (POD5[prefix], run_dir):
            runs.append([(_read_fields(read), err) for read, err in
                         rio.iter_reads_from_pod5_and_bam(pod5, bam, parse_ref_align=ref_anchored, decode_batch=decode_batch)])
        assert len(runs[0]) == (14 if bam is not dirty else 13) and len(runs[1]) == len(runs[0])  # (dirty: 15 records, one secondary, one absent)
        for (a, a_err), (b, b_err) in zip(*runs):
            assert a_err == b_err and a == b


def test_a_bam_whose_batches_span_both_files(run_dir, tmp_path):
    """The records of both BAMs interleaved under can_mappings.bam's header (the reference tables are equal): every batch of
    four holds reads of both files; per read the arrays are those of the two single-file runs."""
    import torch

    from remora_amd import io as rio

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert rio.bam_reference_names(BAM["can"]) == rio.bam_reference_names(BAM["mod"])
    recs = {p: list(rio.iter_bam_records(BAM[p])) for p in ("can", "mod")}
    mixed = str(tmp_path / "mixed.bam")
    order = []
    with rio.BamWriter(mixed, rio.read_bam_header_bytes(BAM["can"])) as w:
        for a, b in zip(recs["can"], recs["mod"]):
            for r in (a, b):
                w.write(struct.pack("<i", len(r.raw)) + bytes(r.raw))
                order.append(r.query_name)

    def per_read(pod5, bam, ref_anchored):
        out = []
        for ib in rio.iter_ingest_batches(pod5, bam, batch=4, ref_anchored=ref_anchored):
            assert isinstance(ib, rio.IngestBatch) and ib.dr is not None
            dr = ib.dr
            dacs, s2s, iseq = dr.dacs.cpu().numpy(), dr.s2s.cpu().numpy(), dr.iseq.cpu().numpy()
            shift, scale = dr.shift.cpu().numpy(), dr.scale.cpu().numpy()
            names = [r.query_name for r in ib.records(ib.rb)]
            good_at = {int(k): g for g, k in enumerate(ib.good.tolist())}
            for k, i in enumerate(ib.keep.tolist()):
                g = good_at.get(k)
                if g is None:
                    out.append((names[i], ib.err[k]))
                    continue
                out.append((names[i], None, dacs[dr.sig_off[g] : dr.sig_off[g + 1]].tobytes(),
                            s2s[dr.seq_off[g] + g : dr.seq_off[g + 1] + g + 1].tobytes(), iseq[dr.seq_off[g] : dr.seq_off[g + 1]].tobytes(),
                            shift[g].tobytes(), scale[g].tobytes(), float(ib.cal_off[g]), float(ib.cal_scale[g]),
                            ib.seq[ib.seq_off[g] : ib.seq_off[g + 1]]))
        return out

    for ref_anchored in (False, True):
        union = {}
        for p in ("can", "mod"):
            for item in per_read(POD5[p], BAM[p], ref_anchored):
                assert item[0] not in union
                union[item[0]] = item
        got = per_read(run_dir, mixed, ref_anchored)
        assert [item[0] for item in got] == order and len(got) == 28
        assert all(item == union[item[0]] for item in got)
        # and neither single file holds the other's reads: half the records of every batch are passed over there
        assert [item[0] for item in per_read(POD5["can"], mixed, ref_anchored)] == order[0::2]


def test_infer_cli_writes_the_single_file_output_from_the_directory(run_dir, tmp_path):
    """`python -m remora_amd infer from_pod5_and_bam DIR BAM`: the output file of the run on the single POD5 file, byte for
    byte; with --procs-per-gpu 2 (every rank builds its own index) the same records."""
    from conftest import golden
    from remora_amd import io as rio
    from test_gpu_shard import TWO, _mint, _remora

    pt = _mint(tmp_path, golden("real_reads_can.npz"))
    outs = {}
    for name, pod5, extra, env in (("file", POD5["can"], [], None), ("dir", run_dir, [], None),
                                   ("procs", run_dir, ["--procs-per-gpu", "2"], TWO)):
        outs[name] = str(tmp_path / f"{name}.bam")
        text = _remora("infer", "from_pod5_and_bam", pod5, BAM["can"], "--model", pt, "--reads-per-batch", "4", "--out-bam", outs[name], *extra,
                       env_extra=env)
        assert "called 14 reads" in text
    assert open(outs["dir"], "rb").read() == open(outs["file"], "rb").read()
    one, two = list(rio.iter_bam_records(outs["file"])), list(rio.iter_bam_records(outs["procs"]))
    assert len(one) == len(two) == 14 and all(bytes(a.raw) == bytes(b.raw) for a, b in zip(one, two))
    assert sum("MM" in dict(r.tags) for r in one) == 14


def test_dataset_prepare_from_the_directory(run_dir, tmp_path):
    import torch

    from remora_amd import io as rio
    from remora_amd import prepare_train_data as ptd
    from remora_amd.refine_signal_map import SigMapRefiner
    from remora_amd.util import Motif

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    table = os.path.join(DATA, "levels_4mer.txt")
    for prefix, mod_base in (("mod", ("m", "5mC")), ("can", None)):
        dirs = []
        for name, pod5 in (("file", POD5[prefix]), ("dir", run_dir)):
            out = str(tmp_path / f"{prefix}_{name}")
            np.random.seed(11)
            ds, errs = ptd.extract_chunk_dataset(
                bam_path=BAM[prefix], pod5_path=pod5, out_path=out, mod_base=mod_base, mod_base_control=mod_base is None, motifs=[Motif("CG", 0)],
                focus_ref_pos=None, chunk_context=(50, 50), min_samps_per_base=5, max_chunks_per_read=15, pa_scaling=None,
                sig_map_refiner=SigMapRefiner(kmer_model_filename=table, do_rough_rescale=True, scale_iters=0, do_fix_guage=True),
                kmer_context_bases=(4, 4), base_start_justify=False, offset=0, num_reads=None, reads_per_batch=5)
            assert ds.size > 50
            dirs.append((out, dict(errs)))
        (a, a_errs), (b, b_errs) = dirs
        assert a_errs == b_errs and sorted(os.listdir(a)) == sorted(os.listdir(b))
        for name in os.listdir(a):
            assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name


def test_kmer_levels_from_the_directory(run_dir):
    """io.get_site_kmer_levels (`analyze estimate_kmer_levels`), in one pass and in ranges (the directory is opened once per pass)."""
    import torch

    from remora_amd import io as rio
    from remora_amd.refine_signal_map import SigMapRefiner

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    table = os.path.join(DATA, "levels_4mer.txt")
    refiner = SigMapRefiner(kmer_model_filename=table, scale_iters=0, do_fix_guage=True, sd_params=[4, 3, 0.5])
    want = rio.get_site_kmer_levels(POD5["can"], BAM["can"], refiner, (1, 2), min_cov=3)
    _, span = rio.count_site_level_reads(BAM["can"])
    for kwargs in ({}, {"max_resident_bases": int(span.sum()) // 2 - 1}):
        got = rio.get_site_kmer_levels(run_dir, BAM["can"], refiner, (1, 2), min_cov=3, **kwargs)
        assert list(got) == list(want) and sum(v.size for v in want.values()) > 0
        for kmer in want:
            assert got[kmer].tobytes() == want[kmer].tobytes(), kmer


def test_the_dataset_answers_by_id_like_the_file(run_dir):
    """get / get_many / signal_rows / calibration / `in` / len / iteration: through the index, the values of the files."""
    import torch

    from remora_amd import io as rio

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    ds = rio.open_pod5(run_dir)
    single = {p: rio.Pod5File(POD5[p]) for p in ("can", "mod")}
    assert len(ds) == 28 and ds.n_dropped == 0 and ds.repeated_ids() == set() and ds._ids is None
    ids = single["can"].read_ids + single["mod"].read_ids
    assert ds.read_ids == ids
    for p in ("can", "mod"):
        f = single[p]
        for rid in f.read_ids[::5]:
            assert rid in ds and rid.upper() in ds
            assert ds.signal_rows(rid) == f.signal_rows(rid) and ds.calibration(rid) == f.calibration(rid)
            a, b = ds.get(rid), f.get(rid)
            assert a.read_id == b.read_id and np.array_equal(a.signal, b.signal) and a.signal.dtype == b.signal.dtype
            assert (a.calibration_offset, a.calibration_scale) == (b.calibration_offset, b.calibration_scale)
    mixed = [ids[20], ids[1], ids[27], ids[1]]
    for a, rid in zip(ds.get_many(mixed), mixed):
        b = (single["can"] if rid in single["can"] else single["mod"]).get(rid)
        assert a.read_id == rid and np.array_equal(a.signal, b.signal)
    for absent in ("0" * 36, "", "not-a-read", ids[0][:-1], ids[0] + "0", None, 7, ids[0].encode()):
        assert absent not in ds
    with pytest.raises(KeyError):
        ds.get("0" * 36)
    assert [r.read_id for r in ds] == ids
    # rows_of_names: the names of a batch as they stand in its blob
    blob = "".join(ids[::-1]).encode() + b"zz"
    off = np.concatenate([36 * np.arange(29), [36 * 28 + 2]]).astype(np.int64)
    assert ds.rows_of_names(blob, off).tolist() == list(range(27, -1, -1)) + [-1]


CHILD = r"""
import logging, os, resource, sys
import numpy as np
run, bam, single = sys.argv[1:4]
resource.setrlimit(resource.RLIMIT_NOFILE, (256, 256))
sys.path.insert(0, os.getcwd())
seen = []
class Keep(logging.Handler):
    def emit(self, record):
        seen.append(record.getMessage())
logging.getLogger("Remora").addHandler(Keep(level=logging.WARNING))
from remora_amd import io as rio
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from test_gpu_pod5_dataset import _assert_same_batches, _ingest
ds = rio.open_pod5(run)
assert len(ds.files) == 1100 and ds.n_rows == 1100 * 14
assert len(ds) == 28, len(ds)
assert len(seen) == 1 and seen[0].startswith(f"{1100 * 14 - 28} POD5 reads repeat"), seen
ids = rio.Pod5File(single).read_ids + rio.Pod5File(single.replace("can_reads", "mod_reads")).read_ids
rows = ds._rows_of_ids(ids)
assert rows.tolist() == list(range(28)), rows.tolist()  # every id resolves into the first two files
assert ds.repeated_ids() == set(ids)
for ref_anchored in (False, True):
    _assert_same_batches(_ingest(ds, bam, 5, ref_anchored), _ingest(single, bam, 5, ref_anchored))
assert len(seen) == 1, seen
assert len(os.listdir("/proc/self/fd")) < 256
print("CHILD OK")
"""


def test_a_run_of_1100_files_opens_under_a_descriptor_limit_of_256(tmp_path):
    """1100 links alternating between the two fixtures, opened by a fresh process whose RLIMIT_NOFILE is 256: no descriptor is
    kept per file; 1100 x 14 - 28 entries repeat an id of the first two files and are dropped with ONE warning; the ingest of
    can_mappings.bam is what the single file gives."""
    run = tmp_path / "big"
    run.mkdir()
    for k in range(1100):
        os.symlink(POD5["can" if k % 2 == 0 else "mod"], run / f"reads_{k:04d}.pod5")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-c", CHILD, str(run), BAM["can"], POD5["can"]], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=env)
    assert r.returncode == 0 and "CHILD OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_refusals_through_the_ingest(tmp_path):
    from remora_amd import io as rio

    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(rio.RemoraError) as e:
        next(iter(rio.iter_ingest_batches(str(empty), BAM["can"])))
    assert str(e.value) == f"no *.pod5 files in directory {empty}"
    text = tmp_path / "text"
    text.mkdir()
    (text / "only.pod5").write_text("signal, they said\n")
    for opener in (lambda: next(iter(rio.iter_ingest_batches(str(text), BAM["can"]))),
                   lambda: next(iter(rio.iter_reads_from_pod5_and_bam(str(text), BAM["can"])))):
        with pytest.raises(rio.RemoraError) as e:
            opener()
        assert str(e.value) == f"{text / 'only.pod5'} is not a POD5 file"


def test_region_api_and_duplex_pairs_take_the_directory(run_dir, tmp_path):
    """The pair pass of the region API (metrics and read extraction) and DuplexPairsBuilder open their POD5 argument the same
    way: the directory gives the single files' values."""
    import shutil

    import torch

    from duplex_fixture import PAIRS, SIMPLEX_BAM, duplex_pod5
    from remora_amd import io as rio

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    rec = next(r for r in rio.iter_bam_records(BAM["can"]) if not r.flag & 16)
    reg = rio.RefRegion(rec.reference_name, "+", rec.reference_start + 20, rec.reference_start + 70)
    want, want_recs = rio.get_ref_reg_samples_metrics(reg, [(POD5[p], BAM[p]) for p in ("can", "mod")], metric="dwell_trimmean_trimsd")
    got, got_recs = rio.get_ref_reg_samples_metrics(reg, [(run_dir, BAM[p]) for p in ("can", "mod")], metric="dwell_trimmean_trimsd")
    assert len(want) == 2 and [[r.query_name for r in rs] for rs in got_recs] == [[r.query_name for r in rs] for rs in want_recs]
    for g, w in zip(got, want):
        assert list(g) == list(w) and all(g[k].tobytes() == w[k].tobytes() and g[k].shape[0] >= 1 for k in w)
    (w_rr,), _ = rio.get_reads_reference_regions(reg, [(POD5["can"], BAM["can"])], max_reads=None)
    (g_rr,), _ = rio.get_reads_reference_regions(reg, [(rio.open_pod5(run_dir), BAM["can"])], max_reads=None)
    assert len(w_rr) >= 1 and [r.read_id for r in g_rr] == [r.read_id for r in w_rr]
    assert all(a.norm_signal.tobytes() == b.norm_signal.tobytes() and a.seq == b.seq for a, b in zip(g_rr, w_rr))
    # duplex: the simplex reads of the pairs, from a directory that holds the duplex run's file beside another
    single = duplex_pod5(tmp_path)
    both = tmp_path / "duplex_run"
    both.mkdir()
    shutil.copy(POD5["can"], both / "0_other.pod5")
    os.symlink(single, both / "duplex_reads.pod5")
    pairs = [tuple(line.split()) for line in open(PAIRS)]
    made = []
    for pod5 in (single, str(both)):
        simplex = rio.ReadIndexedBam(SIMPLEX_BAM, skip_non_primary=True, req_tags={"mv"})
        with rio.DuplexPairsBuilder(simplex, pod5) as builder:
            made.append(builder.make_read_pairs(pairs + [("0" * 36, pairs[0][1])]))
    assert [err for _, err in made[0]] == [None, None, "duplex pair read id(s) missing from pod5"] == [err for _, err in made[1]]
    for (a, _), (b, _) in zip(made[0][:2], made[1][:2]):
        for x, y in zip(a, b):
            assert x.read_id == y.read_id and np.array_equal(x.dacs, y.dacs) and np.array_equal(x.query_to_signal, y.query_to_signal)
            assert (x.shift_dacs_to_pa, x.scale_dacs_to_pa) == (y.shift_dacs_to_pa, y.scale_dacs_to_pa)
