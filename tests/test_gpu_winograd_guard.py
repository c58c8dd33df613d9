"""GPU tests of the Winograd guard (include/remora_hip.h, rmr_model_numerics): every fp32 model with a
Winograd layer (merge_conv1 of models/ConvLSTM_w_ref.py:36-37,50, merge_conv1 / merge_conv2 of models/Conv_w_ref.py:35-38,54-55
and the stride-3 layers in front of them) is screened at load on a fixed probe batch; the record is there and quiet for the
models the project ships tests for, a tripped guard really selects the direct kernels in every forward entry, non-finite
weights trip it, the probe leaves no trace on the engine, and networks the reference TRAINED pass through both forms."""
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 2e-5  # the guard's default: what tests/test_gpu_wino.py allows the two forms on the reference-generated models
MD = dict(chunk_context=(50, 50), kmer_context_bases=(4, 4), motifs=[("CG", 0)], mod_bases=["m"], mod_long_names=["5mC"],
          can_base="C", base_start_justify=False, offset=0, sig_map_refiner=None)


def _direct(fn):
    os.environ["RMR_WINOGRAD"] = "0"
    try:
        return fn()
    finally:
        del os.environ["RMR_WINOGRAD"]


def _profile_of(eng, fn):
    eng.profile_reset()
    eng.profile_enable(True)
    out = fn()
    eng.profile_enable(False)
    return out, eng.profile()


def _same_bits(a, b):
    a, b = (x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _golden_model(name, dtype="fp32"):
    from oracle import oracle as O
    from remora_amd.model_util import model_from_state

    g = np.load(os.path.join(GOLD, f"model_{name}.npz"))
    size, kb, ka, L, num_out = (int(x) for x in g["params"])
    md = dict(chunk_context=(L // 2, L - L // 2), kmer_context_bases=(kb, ka))
    return model_from_state(O.state_from_npz(g), md, device=0, dtype=dtype), md, g, (kb, ka)


@pytest.fixture(scope="module")
def chunks():
    from remora_amd import synth

    return synth.synth_chunks_config("C100", 1000, shard=77)


@pytest.fixture(scope="module")
def dense(chunks):
    from oracle import oracle as O

    return O.compute_encoded_kmer_batch(4, 4, chunks["sequence"], chunks["sequence_to_signal_mapping"], chunks["sequence_lengths"])


# ---- the record exists and is quiet ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["convlstm_s64_l100_o2", "conv_s64_l100_o2", "convlstm_s64_l200_o3"])
def test_golden_models_are_screened_and_keep_the_winograd_kernels(name, caplog):
    with caplog.at_level(logging.INFO, logger="Remora"):
        model, md, _, _ = _golden_model(name)
    rec = model.numerics
    print(name, rec)
    assert rec["checked"] == 1 and rec["winograd"] == 1 and rec["probe_chunks"] == 256, rec
    assert 0 < rec["max_abs_diff"] <= TOL, rec
    assert rec["nonfinite"] == 0 and rec["tol"] == np.float32(TOL), rec
    assert md["winograd"] == "winograd"
    assert not [r for r in caplog.records if "Winograd" in r.getMessage()], "a quiet guard logs nothing"


@pytest.mark.parametrize("name,dtype", [("convlstm_s128_l100_o2", "fp32"), ("convlstm_s64_l100_o2", "bf16"), ("convlstm_s64_l100_o2", "f16x3")])
def test_models_without_a_winograd_layer_are_not_screened(name, dtype):
    model, md, _, _ = _golden_model(name, dtype)
    rec = model.numerics
    assert rec["checked"] == 0 and rec["winograd"] == 0 and rec["probe_chunks"] == 0, rec
    assert md["winograd"] == "n/a"
    assert model.check_winograd(0.0)["checked"] == 0  # asking again does not make a layer appear


# ---- a tripped guard really selects the direct kernels ----------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["chunks", "dense", "read"])
def test_tripped_guard_selects_the_direct_kernels_in_every_entry(entry, chunks, dense):
    from remora_amd import synth
    from remora_amd.data_chunks import RemoraRead
    from remora_amd.inference import call_read_mods
    from remora_amd.model_util import model_from_state

    md = dict(MD)
    model = model_from_state(synth.synth_state("conv_lstm", 64, 9, 2, seed=0), md, device=0, dtype="fp32")
    eng = model.engine
    assert model.numerics["checked"] == 1 and model.numerics["winograd"] == 1, model.numerics

    if entry == "read":
        r = synth.synth_read(400)
        reads = [RemoraRead(dacs=r["dacs"], shift=r["shift"], scale=r["scale"], seq_to_sig_map=r["seq_to_sig_map"],
                            int_seq=r["int_seq"], read_id="guard"), RemoraRead.test_read(nbases=40)]
        runs = [lambda rd=rd: call_read_mods(rd, model, md)[0] for rd in reads]
    else:
        runs = []
        for n in (1, 17, 1000):
            if entry == "chunks":
                args = [chunks[k][:n] for k in ("signal", "sequence", "sequence_to_signal_mapping", "sequence_lengths")]
                runs.append(lambda args=args: model.infer_chunks(*args, (4, 4)))
            else:
                runs.append(lambda n=n: model(chunks["signal"][:n], dense[:n]).numpy())
    for k, run in enumerate(runs):
        before, prof = _profile_of(eng, run)
        assert before.shape[0] > 0 and "conv_merge1" in prof and "winograd_form" in prof, sorted(prof)
        env_direct = _direct(run)
        rec = model.check_winograd(tol=0.0)
        assert rec["checked"] == 1 and rec["winograd"] == 0 and rec["tol"] == 0.0 and rec["max_abs_diff"] > 0, rec
        assert eng.profile() == prof, "the probe left records in the profiler"
        tripped, tprof = _profile_of(eng, run)
        # merge_conv1 ran, and no kernel of the call was launched in a Winograd form
        assert "conv_merge1" in tprof and "winograd_form" not in tprof, sorted(tprof)
        assert _same_bits(tripped, env_direct), (entry, k, "a tripped guard and RMR_WINOGRAD=0 must run the same kernels")
        if k != len(runs) - 1 or entry != "read":  # (test_read: a silent signal, on which the forms may agree to the bit)
            assert not _same_bits(tripped, before), (entry, k)
        rec = model.check_winograd(tol=None)
        assert rec["winograd"] == 1 and rec["tol"] == np.float32(TOL), rec
        assert _same_bits(run(), before), (entry, k, "restoring the default brings the Winograd kernels back")
    assert model.check_winograd(float("inf"))["winograd"] == 1


# ---- non-finite weights trip it ------------------------------------------------------------------------------------------
def test_non_finite_weights_trip_the_guard(chunks, caplog):
    from remora_amd import synth
    from remora_amd.model_util import model_from_state

    state = synth.synth_state("conv_lstm", 64, 9, 2, seed=0)
    state["merge_conv1.weight"] = state["merge_conv1.weight"].copy()
    state["merge_conv1.weight"][3, 17, 2] = np.inf
    md = dict(MD)
    with caplog.at_level(logging.INFO, logger="Remora"):
        model = model_from_state(state, md, device=0, dtype="fp32")
    rec = model.numerics
    assert rec["checked"] == 1 and rec["winograd"] == 0 and rec["nonfinite"] > 0, rec
    assert md["winograd"] == "direct"
    lines = [r.getMessage() for r in caplog.records if r.levelno == logging.INFO and "Winograd" in r.getMessage()]
    assert len(lines) == 1 and "max_abs_diff" in lines[0] and "tol" in lines[0] and "conv_lstm" in lines[0], lines
    args = [chunks[k][:17] for k in ("signal", "sequence", "sequence_to_signal_mapping", "sequence_lengths")]
    out = model.infer_chunks(*args, (4, 4))
    assert _same_bits(out, _direct(lambda: model.infer_chunks(*args, (4, 4))))
    assert not np.isfinite(out).all()  # the network really is broken; the guard only keeps the transform out of it
    assert model.check_winograd(float("inf"))["winograd"] == 0  # no tolerance admits non-finite logits


# ---- the probe leaves no trace ---------------------------------------------------------------------------------------------
def test_probe_leaves_the_engine_as_it_found_it(chunks):
    from remora_amd import synth
    from remora_amd.engine import Engine
    from remora_amd.model_util import model_from_state

    eng = Engine(0, use_torch_stream=False)
    eng.set_subbatch(7)
    eng.profile_enable(True)
    state = synth.synth_state("conv_lstm", 64, 9, 2, seed=3)
    model = model_from_state(state, dict(MD), engine=eng, dtype="fp32")
    assert model.numerics["checked"] == 1
    assert eng.profile() == {}, "the probe's launches reached the profiler"
    args = [chunks[k][:21] for k in ("signal", "sequence", "sequence_to_signal_mapping", "sequence_lengths")]
    out = model.infer_chunks(*args, (4, 4))
    prof = eng.profile()
    assert prof["conv_merge1"][1] == 3, prof  # 21 chunks in sub-batches of 7: the setting survived, profiling is still on
    assert "probe_max_diff" not in prof and "probe_nonfinite" not in prof
    eng.profile_enable(False)
    other = model_from_state(state, dict(MD), engine=eng, dtype="fp32")
    assert other.numerics == model.numerics
    assert _same_bits(other.infer_chunks(*args, (4, 4)), out)
    eng.set_subbatch(0)
    assert _same_bits(model.infer_chunks(*args, (4, 4)), out)


# ---- goldens from trained networks ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["convlstm_s64_l100_o2_trained", "conv_s64_l100_o2_trained"])
def test_trained_golden_models_through_both_forms(name):
    """tools/gen_golden.py --only trained: the reference's own network, trained on the CPU until it separates synthetic
    labelled chunks (held-out accuracy >= 0.9, BatchNorm statistics earned in train mode), exported and reloaded; its logits
    through the default path and the direct form within the project's 1e-4, the two forms within 2e-5 of each other, and the
    guard keeps the Winograd kernels."""
    model, md, g, kcb = _golden_model(name)
    args = (g["sigs"], g["seqs"], g["maps"], g["lens"], kcb)
    out = model.infer_chunks(*args)
    direct = _direct(lambda: model.infer_chunks(*args))
    e_out, e_dir, e_forms = (float(np.abs(a - b).max()) for a, b in ((out, g["logits"]), (direct, g["logits"]), (out, direct)))
    print(name, model.numerics, "default vs reference", e_out, "direct vs reference", e_dir, "winograd vs direct", e_forms)
    assert e_out <= 1e-4, (name, e_out)
    assert e_dir <= 1e-4, (name, e_dir)
    assert e_forms <= TOL, (name, e_forms)
    assert model.numerics["winograd"] == 1 and md["winograd"] == "winograd", model.numerics
