"""Duplex modified-base calling on the GPU: DuplexReadModCaller and `infer duplex_from_pod5_and_bam` on the reference's fixture
pairs (tests/golden/data: two pairs of 7.8 kb and 24.5 kb, one duplex record forward and three reverse) with the golden CG 5mC
model - the reference test's assertions (tests/test_duplex.py:263-298), the composition of parts that have tests of their own,
the command line file to file, and the batch path against the per-read objects."""
import struct

import numpy as np
import pytest

import duplex_restate as R
from duplex_fixture import DUPLEX_BAM, PAIRS, SIMPLEX_BAM, duplex_pod5

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """(model, metadata, model file, POD5 path, [(template id, complement id)], [DuplexRead] made by the batch path)."""
    import torch

    from oracle import oracle as O
    from remora_amd import io as rio
    from remora_amd.model_util import load_model
    from test_gpu_parity import _mint_pt, _real_reads_golden

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    tmp = tmp_path_factory.mktemp("duplex")
    pt = _mint_pt(tmp, _real_reads_golden("can"), O)
    model, md = load_model(pt, device=0)
    pod5 = duplex_pod5(tmp)
    pairs = [tuple(line.split()) for line in open(PAIRS)]
    simplex = rio.ReadIndexedBam(SIMPLEX_BAM, skip_non_primary=True, req_tags={"mv"})
    duplex = rio.ReadIndexedBam(DUPLEX_BAM, skip_non_primary=True, req_tags=set(), read_id_converter=lambda k: k.split(";")[0])
    builder = rio.DuplexPairsBuilder(simplex, pod5)
    read_pairs = builder.make_read_pairs(pairs)
    assert [err for _, err in read_pairs] == [None, None]
    items = [(reads[0], reads[1], duplex.get_first_alignment(p[0])) for (reads, _), p in zip(read_pairs, pairs)]
    made = rio.duplex_reads_batch(items)
    assert [err for _, err in made] == [None, None]
    return dict(model=model, md=md, pt=pt, pod5=pod5, pairs=pairs, items=items, duplex_reads=[d for d, _ in made], tmp=tmp)


def test_reference_assertions_on_call_duplex_read_mod_probs(env):
    """tests/test_duplex.py:263-298."""
    from remora_amd.inference import DuplexReadModCaller
    from remora_amd.io import revcomp

    caller = DuplexReadModCaller(env["model"], env["md"])
    motifs = [m[0] for m in env["md"]["motifs"]]
    assert motifs == ["CG"] and [d.is_reverse_mapped for d in env["duplex_reads"]] == [True, False]
    for duplex_read in env["duplex_reads"]:
        dat = caller.call_duplex_read_mod_probs(duplex_read)
        seq = duplex_read.duplex_basecalled_sequence
        want = revcomp(seq) if duplex_read.is_reverse_mapped else seq
        assert dat["read_sequence"] == want
        assert len(dat["template_positions"]) == len(dat["template_probs"]) > 100
        assert len(dat["complement_positions"]) == len(dat["complement_probs"]) > 100
        for p in dat["template_positions"]:
            assert want[p:p + 2] in motifs
        for p in dat["complement_positions"]:
            assert want[p - 1:p + 1] in motifs


def test_result_is_the_composition_of_tested_parts(env):
    """The 7.8 kb pair: the restatement's alignment (the C++ twin of tests/duplex_restate.py) -> its mapping -> map_ref_to_signal
    -> into_remora_read -> the per-read call_read_mods.  Positions are equal; so are the probabilities, bit for bit: the batch
    path and the per-read path run the same chunks through the same fp32 kernels, which is what
    test_gpu_parity.test_batched_call_reads_mods_matches_single_read_api holds them to."""
    from remora_amd import data_chunks as DC
    from remora_amd.inference import DuplexReadModCaller, call_read_mods
    from remora_amd.io import revcomp

    k = [len(d.duplex_basecalled_sequence) for d in env["duplex_reads"]].index(7782)
    template, complement, rec = env["items"][k]
    duplex_read = env["duplex_reads"][k]
    first, second = (complement, template) if rec.is_reverse else (template, complement)
    aligns = [(first.seq, rec.query_sequence), (second.seq, revcomp(rec.query_sequence))]
    parts = []
    for read, (_, duplex_seq), w in zip((first, second), aligns, R.align_cpp(aligns, R.build_cpp(env["tmp"]))):
        assert w["status"] == R.ST_OK
        anchored = read.copy()
        anchored.query_to_signal = DC.map_ref_to_signal(query_to_signal=read.query_to_signal, ref_to_query_knots=R.mapping(w))
        anchored.seq = duplex_seq[w["ref_start"]:w["ref_end"]]
        probs, _, pos = call_read_mods(anchored.into_remora_read(False), env["model"], env["md"], return_mod_probs=True)
        parts.append((probs, pos + w["ref_start"]))
    if rec.is_reverse:
        parts = parts[::-1]
    dat = DuplexReadModCaller(env["model"], env["md"]).call_duplex_read_mod_probs(duplex_read)
    assert np.array_equal(dat["template_positions"], parts[0][1])
    assert np.array_equal(dat["complement_positions"], len(rec.query_sequence) - parts[1][1] - 1)
    assert np.array_equal(dat["template_probs"], parts[0][0]) and np.array_equal(dat["complement_probs"], parts[1][0])


def _records(path):
    from remora_amd import io as rio

    return list(rio.iter_bam_records(path))


def _without_mod_tags(rec):
    tag_region = bytes(rec.raw[rec.tags_offset:])
    return bytes(rec.raw[:rec.tags_offset]) + b"".join(tag_region[s:e] for name, s, e in rec.tag_spans if name not in ("MM", "ML"))


def test_cli_file_to_file(env, tmp_path):
    from remora_amd.__main__ import main
    from remora_amd.inference import DuplexReadModCaller

    out = str(tmp_path / "out.bam")
    base = ["infer", "duplex_from_pod5_and_bam", env["pod5"], SIMPLEX_BAM, DUPLEX_BAM]
    tail = ["--model", env["pt"], "--out-bam", out, "--device", "0", "--num-extract-alignment-workers", "2"]
    assert main(base + [PAIRS] + tail) == 0
    got = _records(out)
    inputs = {}
    for r in _records(DUPLEX_BAM):
        inputs.setdefault(r.query_name.split(";")[0], r)
    # one record per valid pair, in the order of the pairs file; everything but MM / ML as in the input record
    assert [r.query_name.split(";")[0] for r in got] == [t for t, _ in env["pairs"]]
    caller = DuplexReadModCaller(env["model"], env["md"])
    for r, duplex_read in zip(got, env["duplex_reads"]):
        src = inputs[r.query_name.split(";")[0]]
        assert _without_mod_tags(r) == _without_mod_tags(src)
        mm, ml = r.get_tag("MM"), r.get_tag("ML")
        assert mm.startswith("C+m?,") and ";G-m?," in mm and mm.count(";") == 2
        dat = caller.call_duplex_read_mod_probs(duplex_read)
        assert len(ml) == len(dat["template_positions"]) + len(dat["complement_positions"])
        # the batch path gives the bytes of the per-read objects
        mm_tag, ml_tag = caller.call_duplex_read_mods(duplex_read)
        assert mm_tag == "MM:Z:" + mm and ml_tag == "ML:B:C," + ",".join(str(int(x)) for x in ml)
    # --num-reads 1
    one = str(tmp_path / "one.bam")
    assert main(base + [PAIRS] + tail[:3] + [one] + ["--num-reads", "1", "--reads-per-batch", "1"]) == 0
    assert [r.raw for r in _records(one)] == [got[0].raw]
    # a pair whose complement id the simplex BAM holds (a renamed copy of the record) and the POD5 does not: tallied under the
    # reference's text, the rest written
    from remora_amd import io as rio
    from remora_amd.inference import infer_duplex

    ghost = "0" * 8 + env["pairs"][1][1][8:]
    bam = str(tmp_path / "simplex_plus.bam")
    with rio.BamWriter(bam, rio.read_bam_header_bytes(SIMPLEX_BAM)) as w:
        for r in _records(SIMPLEX_BAM):
            raw = bytes(r.raw)
            w.write(struct.pack("<i", len(raw)) + raw)
            if r.query_name == env["pairs"][1][1]:
                raw = raw[:32] + ghost.encode() + raw[32 + len(ghost):]
                w.write(struct.pack("<i", len(raw)) + raw)
    pairs_txt = str(tmp_path / "pairs.txt")
    with open(pairs_txt, "w") as fh:
        fh.write(f"{env['pairs'][1][0]} {ghost}\n{env['pairs'][0][0]}\t{env['pairs'][0][1]}\n")
    out2 = str(tmp_path / "out2.bam")
    errs = infer_duplex(simplex_pod5_path=env["pod5"], simplex_bam_path=bam, duplex_bam_path=DUPLEX_BAM, pairs_path=pairs_txt,
                        model=env["model"], model_metadata=env["md"], out_bam=out2, num_extract_alignment_threads=1,
                        num_duplex_prep_workers=1, num_infer_threads=1)
    assert errs == {"duplex pair read id(s) missing from pod5": 1}
    assert [r.raw for r in _records(out2)] == [got[0].raw]
