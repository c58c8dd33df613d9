"""Dorado-format model directories on the engine (remora_amd.model_util.load_model on a directory): the models of
tests/golden/dorado_export.npz - the reference's export_model_dorado on ConvLSTM_w_ref size 16 (rough-rescale refiner) and
Conv_w_ref size 24 (three outputs; 24 channels run zero-padded at 32) - loaded from directories and run on the existing kernels.

The tolerance everywhere is the project's fp32 gate on reference-generated models, 1e-4 on logits (tests/test_gpu_parity.py).
"""
import logging

import numpy as np
import pytest
import torch

import dorado_cases as DC

pytestmark = pytest.mark.gpu

TOL = 1e-4


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """Per model: the directory of the reference's tensors and config (data only, written by the project's writers), the
    directory our exporter writes from the state, and the model file of the same state."""
    from remora_amd.model_util import export_model_dorado, export_model_torchscript

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    root = tmp_path_factory.mktemp("dorado")
    out = {}
    for tag in DC.TAGS:
        ck = DC.ckpt_of(tag)
        export_model_dorado(ck, None, str(root / f"{tag}_ours"))
        export_model_torchscript(ck, None, str(root / f"{tag}.pt"))
        out[tag] = {"ref": DC.write_reference_dir(tag, root / f"{tag}_ref"), "ours": str(root / f"{tag}_ours"), "pt": str(root / f"{tag}.pt")}
    return out


@pytest.fixture(scope="module")
def loaded(dirs):
    """Every model loaded once: {tag: {kind: (model, metadata, logits on the fixture's chunks)}}."""
    from remora_amd.model_util import load_model

    out = {}
    for tag in DC.TAGS:
        sigs, seqs, maps, lens = DC.chunks_of(tag)
        out[tag] = {}
        for kind, path in dirs[tag].items():
            model, md = load_model(path)
            out[tag][kind] = (model, md, model.infer_chunks(sigs, seqs, maps, lens, DC.KCB))
    return out


@pytest.mark.parametrize("tag", DC.TAGS)
def test_logits_from_directories(tag, loaded):
    """load_model(directory) -> infer_chunks on the fixture's 24 chunks, within 1e-4 of the reference network's logits, from
    the reference's tensors and from our export of the same state; the two directories hold the same bits and give the same
    bits.  The directory's model runs on the kernels of its architecture and width."""
    from remora_amd.engine import HipModel

    want = DC.fixture()[f"{tag}__logits"]
    ref_model, _, ref_logits = loaded[tag]["ref"]
    _, _, our_logits = loaded[tag]["ours"]
    assert isinstance(ref_model, HipModel) and ref_logits.shape == want.shape == (24, ref_model.num_out)
    print(f"{tag}: max|logit - reference| {np.abs(ref_logits - want).max():.3g} (reference tensors), "
          f"{np.abs(our_logits - want).max():.3g} (our export)")
    assert np.isfinite(ref_logits).all()
    assert np.abs(ref_logits - want).max() <= TOL
    assert np.abs(our_logits - want).max() <= TOL
    assert our_logits.tobytes() == ref_logits.tobytes()
    if tag == "conv_s24":
        assert (ref_model.arch, ref_model.size, ref_model.kernel_size, ref_model.num_out) == ("conv_only", 24, 32, 3)
    else:
        assert (ref_model.arch, ref_model.size, ref_model.kernel_size, ref_model.num_out) == ("conv_lstm", 16, 16, 2)
    assert ref_model.dtype == "fp32" and ref_model.chunk_len == 100 and ref_model.kmer_len == 9


@pytest.mark.parametrize("tag", DC.TAGS)
def test_directory_against_model_file(tag, loaded):
    """The directory and the model file of one state, both within 1e-4 of oracle.torch_ref in float64.  They need not agree to
    the bit: the directory's convolutions were folded by fuse_conv_bn_eval in fp32, the model file's are folded by the engine in
    double.  Measured on the MI355X, max |directory - model file|: 2.4e-7 (convlstm_s16), 9.5e-7 (conv_s24); against float64
    the directory is at 3.1e-7 / 1.2e-6 and the model file at 4.9e-7 / 9.4e-7."""
    from oracle import oracle, torch_ref

    sigs, seqs, maps, lens = DC.chunks_of(tag)
    enc = oracle.compute_encoded_kmer_batch(*DC.KCB, seqs, maps, lens)
    net = torch_ref.from_state(DC.state_of(tag)).double()
    with torch.no_grad():
        want = net(torch.from_numpy(sigs).double(), torch.from_numpy(enc).double()).numpy()
    from_dir, from_pt = loaded[tag]["ours"][2], loaded[tag]["pt"][2]
    print(f"{tag}: max|directory - model file| {np.abs(from_dir - from_pt).max():.3g}; against float64: directory "
          f"{np.abs(from_dir - want).max():.3g}, model file {np.abs(from_pt - want).max():.3g}")
    assert np.abs(from_dir - want).max() <= TOL
    assert np.abs(from_pt - want).max() <= TOL


@pytest.mark.parametrize("tag", DC.TAGS)
def test_metadata_equals_the_model_files(tag, loaded):
    from remora_amd.data_chunks import RemoraRead
    from remora_amd.inference import call_read_mods

    dir_model, md, _ = loaded[tag]["ours"]
    pt_model, pt_md, _ = loaded[tag]["pt"]
    assert set(md) == set(pt_md)
    for key in pt_md:
        assert type(md[key]) is type(pt_md[key]), key
    for key in ("chunk_context", "kmer_context_bases", "kmer_len", "chunk_len", "motifs", "can_base", "mod_bases", "mod_long_names", "offset",
                "reverse_signal", "pa_scaling", "motif", "alphabet_str", "base_start_justify", "modified_base_labels", "model_params",
                "model_version", "winograd"):
        assert md[key] == pt_md[key], key
    r, pt_r = md["sig_map_refiner"], pt_md["sig_map_refiner"]
    assert r.center_idx == pt_r.center_idx and r.do_rough_rescale == pt_r.do_rough_rescale and r.is_loaded == pt_r.is_loaded
    if tag == "convlstm_s16":
        assert r.do_rough_rescale and r.center_idx == 2 and r._levels_array.dtype == pt_r._levels_array.dtype
        assert np.array_equal(r._levels_array, pt_r._levels_array)
    else:
        assert r._levels_array is None and pt_r._levels_array is None
    assert md["winograd"] == dir_model.winograd_form
    read_out = [call_read_mods(RemoraRead.test_read(), m, mdata, return_mod_probs=True) for m, mdata in ((dir_model, md), (pt_model, pt_md))]
    (probs, labels, pos), (pt_probs, pt_labels, pt_pos) = read_out
    assert probs.shape == pt_probs.shape and probs.shape[0] > 0 and probs.shape[1] == len(md["mod_bases"])
    assert np.array_equal(pos, pt_pos) and np.array_equal(labels, pt_labels)
    print(f"{tag}: call_read_mods on test_read, {probs.shape[0]} sites, max|dp| {np.abs(probs - pt_probs).max():.3g}")
    assert np.abs(probs - pt_probs).max() <= TOL


def test_trained_to_deployed(tmp_path, caplog):
    """Two training steps, the checkpoint saved as the trainer saves it, `model export` (dorado, the default) through the
    command line, load_model on the directory: the deployed model's logits within 1e-4 of trainer.eval_model()'s."""
    from remora_amd.__main__ import build_parser
    from remora_amd.model_util import load_model
    from remora_amd.train_model import Trainer, save_model
    from test_gpu_train_grads import make_inputs
    from test_gpu_train_steps import checkpoint_of

    tr = Trainer(16, 9, 2, 100, max_batch=8, seed=3)
    sigs, enc, labels = make_inputs(16, 100, 8, 9, 2, seed=5)
    for _ in range(2):
        tr.step(sigs, enc, labels)
    want = tr.eval_model()(sigs, enc).numpy()
    ck = checkpoint_of(tr)
    save_model(tr, ck, str(tmp_path), epoch=0, as_torchscript=False)
    out = str(tmp_path / "deploy")
    args = build_parser().parse_args(["model", "export", str(tmp_path / "model_best.checkpoint"), out])
    with caplog.at_level(logging.INFO, logger="Remora"):
        assert args.func(args) == 0
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING]
    model, md = load_model(out)
    got = model(sigs, enc).numpy()
    print(f"trained -> directory: max|d logit| {np.abs(got - want).max():.3g}")
    assert np.abs(got - want).max() <= TOL
    assert md["mod_bases"] == ["m"] and md["motifs"] == [("CG", 0)] and md["chunk_context"] == [50, 50]


def test_dtypes_are_refused_as_for_a_model_file(dirs):
    from remora_amd import RemoraError
    from remora_amd.model_util import load_torchscript_model

    for tag, dtype in (("conv_s24", "bf16x6"), ("convlstm_s16", "f16")):
        said = []
        for kind in ("pt", "ours"):
            with pytest.raises(RemoraError) as e:
                load_torchscript_model(dirs[tag][kind], dtype=dtype)
            said.append(str(e.value))
        assert said[0] == said[1] and f"dtype={dtype}" in said[0]
    with pytest.raises(RemoraError, match="unknown dtype"):
        load_torchscript_model(dirs["conv_s24"]["ours"], dtype="fp64")


def test_the_environment_chooses_the_dtype_of_a_directory(dirs, monkeypatch):
    from remora_amd import RemoraError
    from remora_amd.model_util import load_model

    monkeypatch.setenv("REMORA_HIP_DTYPE", "f16")
    for kind in ("pt", "ours"):
        with pytest.raises(RemoraError, match="dtype=f16"):
            load_model(dirs["convlstm_s16"][kind])
    monkeypatch.setenv("REMORA_HIP_DTYPE", "f32")
    assert load_model(dirs["convlstm_s16"]["ours"])[0].dtype == "f32"
