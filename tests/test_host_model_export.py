"""CPU-only tests of `model export` / `model inspect`, the dorado-format exporter and reader, and the TOML module behind
`config.toml` (remora_amd/model_util.py, remora_amd/toml_lite.py, remora_amd/__main__.py).  No engine is created anywhere here."""
import json
import logging
import os
import subprocess

import numpy as np
import pytest
import torch

import dorado_cases as DC
from conftest import ROOT

from remora_amd import RemoraError, toml_lite


# ---- 1. export against the reference's --------------------------------------------------------------------------------------
@pytest.mark.parametrize("refiner_object", [False, True], ids=["refine_keys", "refiner_object"])
@pytest.mark.parametrize("tag", DC.TAGS)
def test_export_equals_the_reference_export(tag, refiner_object, tmp_path):
    """export_model_dorado on the fixture's state and metadata: the reference's file names, every tensor bit for bit (the same
    fuse_conv_bn_eval in fp32), and the config the reference handed to toml.dump (creation_date aside, Nones absent, keys in
    its order) - from the `refine_*` keys of a training checkpoint and from the refiner object of a loaded model alike."""
    from remora_amd.model_util import export_model_dorado

    ck = DC.ckpt_of(tag, with_refiner_object=refiner_object)
    if refiner_object:
        for k in [k for k in ck if k.startswith("refine_")]:
            del ck[k]
    state0 = {k: v.clone() for k, v in ck["state_dict"].items()}
    out = str(tmp_path / "exported")
    export_model_dorado(ck, None, out)
    assert sorted(os.listdir(out)) == sorted(DC.fixture()[f"{tag}__files"].tolist())
    want = DC.ref_tensors(tag)
    got = DC.read_dir_tensors(out)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert got[name].tobytes() == want[name].tobytes(), name
    for k, v in ck["state_dict"].items():  # the caller's state is not folded in place
        assert torch.equal(v, state0[k]), k
    for reader in (toml_lite.loads, toml_lite.parse_subset):
        cfg = reader(open(os.path.join(out, "config.toml"), encoding="utf-8").read())
        ref = DC.ref_config(tag)
        assert list(cfg) == list(ref) == ["general", "model_params", "modbases", "refinement"]
        assert isinstance(cfg["general"].pop("creation_date"), str) and ref["general"].pop("creation_date")
        assert cfg == ref
        for table in ref:
            assert list(cfg[table]) == list(ref[table]), table
            assert [type(v) for v in cfg[table].values()] == [type(v) for v in ref[table].values()], table
    assert "pa_scaling" not in cfg["modbases"]
    assert type(cfg["refinement"]["refine_do_rough_rescale"]) is int


def test_export_says_what_the_format_loses(tmp_path, caplog):
    """One INFO line when the directory exists; one WARNING per field the directory does not carry whose value differs from
    what the reader assumes; the files are the same either way."""
    from remora_amd.model_util import export_model_dorado

    ck = DC.ckpt_of("convlstm_s16")
    out = str(tmp_path / "a")
    with caplog.at_level(logging.INFO, logger="Remora"):
        export_model_dorado(ck, None, out)
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING]
    assert not [r for r in caplog.records if "already exists" in r.getMessage()]
    caplog.clear()
    ck.update(base_start_justify=True, refine_scale_iters=2, refine_half_bandwidth=7, model_version=2)
    with caplog.at_level(logging.INFO, logger="Remora"):
        export_model_dorado(ck, None, out)
    assert len([r for r in caplog.records if r.levelno == logging.INFO and "already exists" in r.getMessage()]) == 1
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warned) == 4
    for field in ("base_start_justify", "refine_scale_iters", "refine_half_bandwidth", "model_version"):
        assert sum(f" {field} " in w for w in warned) == 1, field
    got, want = DC.read_dir_tensors(out), DC.ref_tensors("convlstm_s16")
    assert all(got[n].tobytes() == want[n].tobytes() for n in want)


# ---- 2. TOML -----------------------------------------------------------------------------------------------------------------
TRICKY = {"strings": {"quote": 'say "hi"', "backslash": "C:\\models\\x", "both": '\\"', "unicode": "5-méthylcytosine \u4fee\u9970 \U0001f9ec",
                      "control": "tab\there\nnewline\x01\x7f", "empty": "", "hash": "a # b", "key with space": "v"},
          "numbers": {"i": 0, "neg": -17, "big": 2**53 + 1, "f": 0.1, "tiny": 5e-324, "huge": 1.7976931348623157e308, "third": 1 / 3,
                      "negf": -2.5e-7, "whole": 3.0, "inf": float("inf"), "ninf": float("-inf")},
          "flags": {"yes": True, "no": False},
          "arrays": {"pa_scaling": [1.5, -0.25], "names": ["a", 'b"c'], "none": [], "ints": [1, 2, 3]}}


def _same(a, b):
    assert a == b
    for table in a:
        assert list(a[table]) == list(b[table])
        for k in a[table]:
            assert type(a[table][k]) is type(b[table][k]), (table, k)


def test_toml_round_trip():
    for tag in DC.TAGS:
        doc = DC.ref_config(tag)
        _same(toml_lite.parse_subset(toml_lite.dumps(doc)), doc)
        _same(toml_lite.loads(toml_lite.dumps(doc)), doc)
    text = toml_lite.dumps(TRICKY)
    _same(toml_lite.parse_subset(text), TRICKY)
    assert "true" in text and "false" in text and "True" not in text
    assert toml_lite.parse_subset(toml_lite.dumps({"t": {"x": float("nan")}}))["t"]["x"] != toml_lite.parse_subset("[t]\nx = 1.0")["t"]["x"]
    assert toml_lite.dumps({"t": {"a": None, "b": 1}}) == "[t]\nb = 1\n"
    assert toml_lite.parse_subset(toml_lite.dumps({"t": {"n": np.int64(3), "f": np.float32(0.5), "b": np.bool_(True)}})) == \
        {"t": {"n": 3, "f": 0.5, "b": True}}
    for bad in ({"t": {"x": {"nested": 1}}}, {"top": 1}, {"t": {"x": [[1]]}}, {"t": {"x": object()}}):
        with pytest.raises(RemoraError):
            toml_lite.dumps(bad)


def test_toml_writer_output_is_toml_to_a_full_parser():
    try:
        import tomllib as lib
    except ImportError:
        lib = pytest.importorskip("tomli")
    for doc in [DC.ref_config(tag) for tag in DC.TAGS] + [TRICKY]:
        _same(lib.loads(toml_lite.dumps(doc)), doc)


def test_toml_subset_reader_reads_what_model_directories_hold():
    text = ("# a comment\n\ntitle = 'top'\n[general]  # trailing\nmodel = \"conv_lstm\"\nlit = 'C:\\raw\\n'\n\"quoted key\" = 1\n"
            "[modbases]\r\nmod_bases = \"hm\"\noffset = +1\nf = 1e3\ng = -0.5\nh = 1_000\nreverse_signal = false\n"
            "pa = [ 1.5, 2 ,]\nnames = [\"a\", 'b']  # done\nu = \"\\u00e9\\U0001F9EC\"\n")
    doc = toml_lite.parse_subset(text, "x.toml")
    assert doc == {"title": "top", "general": {"model": "conv_lstm", "lit": "C:\\raw\\n", "quoted key": 1},
                   "modbases": {"mod_bases": "hm", "offset": 1, "f": 1000.0, "g": -0.5, "h": 1000, "reverse_signal": False,
                                "pa": [1.5, 2], "names": ["a", "b"], "u": "\u00e9\U0001f9ec"}}
    assert type(doc["modbases"]["f"]) is float and type(doc["modbases"]["h"]) is int


@pytest.mark.parametrize("line,what", [
    ("x = { a = 1 }", "inline table"), ('x = """', "multi-line"), ("x = '''", "multi-line"), ("[a.b]", "nested"), ("[[a]]", "arrays of tables"),
    ("a.b = 1", "dotted"), ("x = 1979-05-27", "1979-05-27"), ("x = 0x1F", "0x1F"), ("x = 01", "01"), ("x = [1, [2]]", "arrays of arrays"),
    ("x = [1,", "not closed"), ('x = "abc', "not closed"), ('x = "\\q"', "escape"), ("x = 1 2", "after the value"), ("x", "expected ="),
    ("x = ", "expected a value"), ("x = True", "True"), ("[a] b", "after the table header"), ("x = 1\nx = 2", "twice"), ("x = 1.", "1."),
    ('x = "\\ud800"', "scalar value")])
def test_toml_subset_reader_refuses_with_file_and_line(line, what):
    text = "# header\n[t]\nok = 1\n" + line + "\n"
    lineno = 3 + len(line.split("\n"))
    with pytest.raises(RemoraError) as e:
        toml_lite.parse_subset(text, "some/config.toml")
    msg = str(e.value)
    assert msg.startswith(f"some/config.toml, line {lineno}: "), msg
    assert what in msg, msg


def test_toml_load_wraps_a_full_parsers_error(tmp_path):
    p = tmp_path / "config.toml"
    p.write_text("[t]\nx = = 1\n")
    with pytest.raises(RemoraError) as e:
        toml_lite.load(p)
    assert str(p) in str(e.value) and "line 2" in str(e.value)


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------
def test_two_motifs_are_refused_with_the_references_message(tmp_path):
    from remora_amd.model_util import export_model_dorado

    ck = DC.ckpt_of("conv_s24")
    ck["motifs"] = [("CG", 0), ("CHG", 0)]
    with pytest.raises(RemoraError, match="^Dorado only supports models with a single motif$"):
        export_model_dorado(ck, None, str(tmp_path / "d"))
    assert not os.path.exists(tmp_path / "d")


def _set_model(path, value):
    cfg = toml_lite.load(os.path.join(path, "config.toml"))
    cfg["general"]["model"] = value
    toml_lite.dump(cfg, os.path.join(path, "config.toml"))


@pytest.mark.parametrize("kind", ["unknown", "conv_lstm_v3"])
def test_other_model_types_are_refused_by_name(kind, tmp_path):
    from remora_amd.model_util import read_dorado_model

    d = DC.write_reference_dir("convlstm_s16", tmp_path / "m")
    _set_model(d, kind)
    with pytest.raises(RemoraError) as e:
        read_dorado_model(d)
    assert repr(kind) in str(e.value) and "'conv_lstm'" in str(e.value) and "'conv_only'" in str(e.value)


def test_tensors_of_the_other_architecture_are_refused(tmp_path):
    from remora_amd.model_util import read_dorado_model

    d = DC.write_reference_dir("conv_s24", tmp_path / "m")
    _set_model(d, "conv_lstm")
    with pytest.raises(RemoraError) as e:
        read_dorado_model(d)
    assert "conv_only" in str(e.value) and "general.model = 'conv_lstm'" in str(e.value)


@pytest.mark.parametrize("tag,gone", [("convlstm_s16", "sig_conv2.bias"), ("convlstm_s16", "lstm2.weight_hh_l0"), ("conv_s24", "merge_conv3.weight"),
                                      ("convlstm_s16", "refine_kmer_levels"), ("conv_s24", "fc.weight")])
def test_a_missing_tensor_is_named(tag, gone, tmp_path):
    from remora_amd.model_util import read_dorado_model

    d = DC.write_reference_dir(tag, tmp_path / "m")
    os.remove(os.path.join(d, gone + ".tensor"))
    with pytest.raises(RemoraError) as e:
        read_dorado_model(d)
    assert gone + ".tensor" in str(e.value) and "missing" in str(e.value)


def test_a_whole_missing_layer_is_named(tmp_path):
    from remora_amd.model_util import read_dorado_model

    d = DC.write_reference_dir("convlstm_s16", tmp_path / "m")
    for key in ("weight", "bias"):
        os.remove(os.path.join(d, f"fc.{key}.tensor"))
    with pytest.raises(RemoraError, match=r"fc\.weight\.tensor .* missing \(and 1 more\)"):
        read_dorado_model(d)


def test_directories_and_files_that_are_no_model(tmp_path):
    from remora_amd.model_util import load_model

    (tmp_path / "empty").mkdir()
    with pytest.raises(RemoraError, match="holds no config.toml"):
        load_model(str(tmp_path / "empty"))
    with pytest.raises(RemoraError, match=r"Remora model file \(.*\) not found\."):
        load_model(str(tmp_path / "nothing.pt"))


@pytest.mark.parametrize("tag", DC.TAGS)
def test_read_directory_state_and_metadata(tag, tmp_path, caplog):
    """The state a directory gives the engine: the reference's folded tensors under torch's names, identity BatchNorm
    statistics beside every convolution; the metadata built from the four tables; one INFO line on what is assumed."""
    from remora_amd.engine import _CONV_ORDER, state_to_blob
    from remora_amd.model_util import read_dorado_model
    from remora_amd.refine_signal_map import SigMapRefiner

    d = DC.write_reference_dir(tag, tmp_path / "m")
    with caplog.at_level(logging.INFO, logger="Remora"):
        state, md = read_dorado_model(d)
    lines = [r.getMessage() for r in caplog.records if "does not carry" in r.getMessage()]
    assert len(lines) == 1
    for field in ("base_start_justify", "modified_base_labels", "refine_scale_iters", "refine_algo", "refine_half_bandwidth", "refine_sd_arr",
                  "model_version"):
        assert field in lines[0]
    ref = DC.ref_tensors(tag)
    for name, arr in ref.items():
        if name != "refine_kmer_levels.tensor":
            assert state[name[: -len(".tensor")]].tobytes() == arr.tobytes(), name
    arch, size, kmer_len, num_out, blob = state_to_blob(state)
    ck = DC.ckpt_of(tag)
    assert (arch, size, kmer_len, num_out) == ("conv_lstm" if "lstm" in tag else "conv_only", ck["model_params"]["size"], 9, ck["model_params"]["num_out"])
    for conv, bn in _CONV_ORDER[arch]:
        oc = state[f"{conv}.weight"].shape[0]
        assert np.array_equal(state[f"{bn}.weight"], np.ones(oc, np.float32)) and not state[f"{bn}.bias"].any() and not state[f"{bn}.running_mean"].any()
        assert state[f"{bn}.running_var"].dtype == np.float32 and np.array_equal(state[f"{bn}.running_var"], np.full(oc, np.float32(1 - 1e-5)))
    assert md["chunk_context"] == [50, 50] and md["kmer_context_bases"] == [4, 4] and md["chunk_len"] == 100 and md["kmer_len"] == 9
    assert md["mod_bases"] == ck["mod_bases"] and md["mod_long_names"] == ck["mod_long_names"] and md["motifs"] == ck["motifs"]
    assert md["offset"] == 0 and md["reverse_signal"] is False and md["pa_scaling"] is None and md["base_start_justify"] is False
    assert md["model_params"] == ck["model_params"] and md["model_version"] == 3 and md["modified_base_labels"] is True
    r = md["sig_map_refiner"]
    assert isinstance(r, SigMapRefiner) and not [k for k in md if k.startswith("refine_")]
    if ck["refine_do_rough_rescale"]:
        assert r.do_rough_rescale is True and r.center_idx == ck["refine_kmer_center_idx"] and r.is_loaded and r.kmer_len == 4
        assert r._levels_array.dtype == np.float32 and np.array_equal(r._levels_array, ck["refine_kmer_levels"].astype(np.float32))
        assert r.scale_iters == -1
    else:
        assert not r.is_loaded and not r.do_rough_rescale


def test_a_tensor_file_may_hold_its_tensor_under_any_name_or_as_a_buffer(tmp_path):
    from remora_amd.model_util import load_tensor_file, save_tensor_file

    x = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    save_tensor_file(tmp_path / "a.tensor", x.numpy())
    m = torch.jit.load(str(tmp_path / "a.tensor"))
    assert [n for n, _ in m.named_parameters()] == ["0"] and not next(m.parameters()).requires_grad
    mod = torch.nn.Module()
    mod.register_buffer("weights", x)
    torch.jit.script(mod).save(str(tmp_path / "b.tensor"))
    for f in ("a.tensor", "b.tensor"):
        assert np.array_equal(load_tensor_file(tmp_path / f), x.numpy())
    two = torch.nn.Module()
    two.register_buffer("p", x)
    two.register_buffer("q", x + 1)
    torch.jit.script(two).save(str(tmp_path / "c.tensor"))
    with pytest.raises(RemoraError, match="expected one tensor, found 2"):
        load_tensor_file(tmp_path / "c.tensor")
    (tmp_path / "d.tensor").write_bytes(b"not an archive")
    with pytest.raises(RemoraError, match="not a TorchScript tensor file"):
        load_tensor_file(tmp_path / "d.tensor")


# ---- nets --------------------------------------------------------------------------------------------------------------------
def test_nets_states_both_architectures():
    """from_state builds the architecture detect_arch finds: Conv_w_ref agrees with the oracle's statement of it to the bit
    (same layers, same torch ops), ConvLSTM_w_ref is the class it was; anything else is refused."""
    from oracle import torch_ref
    from remora_amd import nets

    state = DC.state_of("conv_s24")
    net = nets.from_state(state)
    assert type(net) is nets.ConvOnly and not net.training
    ref = torch_ref.from_state(state)
    assert [n for n, _ in net.named_modules()] == [n for n, _ in ref.named_modules()]
    assert list(net.state_dict()) == list(ref.state_dict())
    sigs, seqs, maps, lens = DC.chunks_of("conv_s24")
    rng = np.random.default_rng(0)
    enc = torch.from_numpy(rng.standard_normal((8, 36, 100)).astype(np.float32))
    with torch.no_grad():
        assert torch.equal(net(torch.from_numpy(sigs[:8]), enc), ref(torch.from_numpy(sigs[:8]), enc))
    assert type(nets.from_state(DC.state_of("convlstm_s16"))) is nets.ConvLSTM
    assert type(nets.from_state(nets.build(16, 9, 2, seed=1).state_dict())) is nets.ConvLSTM
    with pytest.raises(RemoraError):
        nets.from_state({k: v for k, v in state.items() if not k.startswith("merge_conv4")})


# ---- 4. checkpoint round trip through the command line ---------------------------------------------------------------------------
class _HeldState:
    """What train_model.save_model asks of a trainer."""

    def __init__(self, state):
        self._state = state

    def state_dict(self):
        return self._state

    def optimizer_state_dict(self):
        return {"state": {}, "param_groups": [{"lr": 1e-3}]}


def _ckpt_save_data(levels=None):
    from remora_amd.refine_signal_map import SigMapRefiner

    refiner = SigMapRefiner() if levels is None else SigMapRefiner(_levels_array=levels, center_idx=2, do_rough_rescale=True)
    return {"epoch": 0, "state_dict": None, "opt": None, "model_path": "/nowhere/ConvLSTM_w_ref.py",
            "model_params": {"size": 16, "kmer_len": 9, "num_out": 2}, "fixed_seq_len_chunks": False, "model_version": 3,
            "chunk_context": (50, 50), "motifs": [("CG", 0)], "num_motifs": 1, "reverse_signal": False, "mod_bases": "m",
            "mod_long_names": ["5mC"], "modified_base_labels": True, "kmer_context_bases": (4, 4), "base_start_justify": False,
            "offset": 0, "pa_scaling": None, **refiner.asdict()}


@pytest.fixture(scope="module")
def trained_dir(tmp_path_factory):
    """model_best.checkpoint and model_best.pt as train_model.save_model writes them, from a hand-built ckpt_save_data."""
    from remora_amd import nets
    from remora_amd.train_model import save_model

    out = tmp_path_factory.mktemp("train")
    levels = DC.fixture()["convlstm_s16__refine_kmer_levels"]
    save_model(_HeldState(nets.build(16, 9, 2, seed=1).state_dict()), _ckpt_save_data(levels), str(out), epoch=4)
    return out


def _run(argv, caplog):
    from remora_amd.__main__ import build_parser

    args = build_parser().parse_args(argv)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="Remora"):
        rc = args.func(args)
    return rc, "\n".join(r.getMessage() for r in caplog.records)


def _attr_lines(text):
    assert "Loaded Remora model attrs\n" in text
    out = {}
    for line in text.split("Loaded Remora model attrs\n", 1)[1].splitlines():
        if " : " in line and line.startswith("  "):
            k, v = line.split(" : ", 1)
            out[k.strip()] = v
    return out


def test_parser_has_the_references_arguments():
    from remora_amd.__main__ import _model_export, _model_inspect, build_parser

    ap = build_parser()
    a = ap.parse_args(["model", "export", "in.checkpoint", "out"])
    assert (a.checkpoint_path, a.output_path, a.model_path, a.format, a.func) == ("in.checkpoint", "out", None, "dorado", _model_export)
    a = ap.parse_args(["model", "export", "in.pt", "out.pt", "--format", "torchscript", "--model-path", "arch.py"])
    assert (a.format, a.model_path) == ("torchscript", "arch.py")
    a = ap.parse_args(["model", "inspect", "in.pt", "--model-path", "arch.py"])
    assert (a.checkpoint_path, a.model_path, a.func) == ("in.pt", "arch.py", _model_inspect)
    with pytest.raises(SystemExit):
        ap.parse_args(["model", "export", "in.pt", "out", "--format", "onnx"])


@pytest.mark.parametrize("name", ["model_best.checkpoint", "model_best.pt"])
def test_inspect_a_checkpoint_and_a_model_file(name, trained_dir, caplog):
    rc, text = _run(["model", "inspect", str(trained_dir / name)], caplog)
    assert rc == 0
    assert ("Loaded model from checkpoint" if name.endswith("checkpoint") else "Loaded a torchscript model") in text
    attrs = _attr_lines(text)
    assert attrs["chunk_context"] in ("(50, 50)", "[50, 50]") and attrs["kmer_context_bases"] in ("(4, 4)", "[4, 4]")
    assert attrs["sig_map_refiner"].startswith("Loaded 4-mer table with 3 central position. Rough re-scaling will be executed.")
    assert attrs["mod_bases"] == "m" and attrs["motifs"] == "[('CG', 0)]"
    assert not [k for k in attrs if k in ("state_dict", "opt") or k.startswith(("refine_", "chunk_context_", "kmer_context_bases_", "motif_",
                                                                                 "mod_long_names_"))]
    assert "state_dict" not in text
    for line in text.split("Loaded Remora model attrs\n", 1)[1].splitlines()[:3]:
        assert line.index(" : ") == 22  # `  {k: >20} : {v}`


@pytest.mark.parametrize("name", ["model_best.checkpoint", "model_best.pt"])
def test_export_to_torchscript(name, trained_dir, tmp_path, caplog):
    from remora_amd.model_util import _META_KEYS, _raw_load_torchscript_model, add_derived_metadata

    out = str(tmp_path / "exported.pt")
    rc, text = _run(["model", "export", str(trained_dir / name), out, "--format", "torchscript"], caplog)
    assert rc == 0 and "Exporting model to TorchScript format" in text
    extra = {"meta.txt": ""}
    script = torch.jit.load(out, _extra_files=extra, map_location="cpu")
    meta = json.loads(extra["meta.txt"])
    assert set(_META_KEYS) <= set(meta)
    state, md = _raw_load_torchscript_model(out)
    want, want_md = _raw_load_torchscript_model(str(trained_dir / "model_best.pt"))
    assert sorted(state) == sorted(want) and all(state[k].tobytes() == want[k].tobytes() for k in want)
    for m in (md, want_md):
        add_derived_metadata(m)
        m.pop("creation_date")
    levels, want_levels = md.pop("sig_map_refiner"), want_md.pop("sig_map_refiner")
    assert md == want_md
    assert np.array_equal(levels._levels_array, want_levels._levels_array) and levels.center_idx == want_levels.center_idx == 2
    sigs = torch.zeros(2, 1, 100)
    with torch.no_grad():
        assert script(sigs, torch.zeros(2, 36, 100)).shape == (2, 2)


@pytest.mark.parametrize("name", ["model_best.checkpoint", "model_best.pt"])
def test_export_to_a_directory_is_the_default(name, trained_dir, tmp_path, caplog):
    from remora_amd.model_util import dorado_tensor_names, read_dorado_model

    out = str(tmp_path / "deploy")
    rc, text = _run(["model", "export", str(trained_dir / name), out], caplog)
    assert rc == 0 and "Exporting model to dorado format" in text
    assert sorted(os.listdir(out)) == sorted([n + ".tensor" for n in dorado_tensor_names("conv_lstm")] + ["refine_kmer_levels.tensor", "config.toml"])
    cfg = toml_lite.load(os.path.join(out, "config.toml"))
    assert cfg["general"]["model"] == "conv_lstm" and cfg["model_params"] == {"size": 16, "kmer_len": 9, "num_out": 2}
    assert cfg["refinement"] == {"refine_do_rough_rescale": 1, "refine_kmer_center_idx": 2}
    assert cfg["modbases"] == {"mod_bases": "m", "offset": 0, "reverse_signal": False, "mod_long_names_0": "5mC", "chunk_context_0": 50,
                               "chunk_context_1": 50, "kmer_context_bases_0": 4, "kmer_context_bases_1": 4, "motif": "CG", "motif_offset": 0}
    state, md = read_dorado_model(out)
    assert np.array_equal(md["sig_map_refiner"]._levels_array, DC.fixture()["convlstm_s16__refine_kmer_levels"].astype(np.float32))
    # both inputs hold the same state: the same files
    again = str(tmp_path / "again")
    other = "model_best.pt" if name.endswith("checkpoint") else "model_best.checkpoint"
    _run(["model", "export", str(trained_dir / other), again], caplog)
    a, b = DC.read_dir_tensors(out), DC.read_dir_tensors(again)
    assert sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_a_conv_w_ref_model_file_goes_through_both_verbs(tmp_path, caplog):
    from remora_amd.model_util import export_model_torchscript

    ck = DC.ckpt_of("conv_s24")
    pt = str(tmp_path / "conv.pt")
    export_model_torchscript(ck, None, pt)
    script = torch.jit.load(pt, map_location="cpu")
    assert "merge_bn4.running_var" in script.state_dict() and "lstm1.weight_ih_l0" not in script.state_dict()
    rc, text = _run(["model", "inspect", pt], caplog)
    attrs = _attr_lines(text)
    assert rc == 0 and attrs["mod_bases"] == "hm" and attrs["sig_map_refiner"] == "No Remora signal refine/map settings loaded"
    assert attrs["model_params"] == "{'size': 24, 'kmer_len': 9, 'num_out': 3}"
    out = str(tmp_path / "deploy")
    rc, _ = _run(["model", "export", pt, out], caplog)
    assert rc == 0
    got, want = DC.read_dir_tensors(out), DC.ref_tensors("conv_s24")
    assert sorted(got) == sorted(want) and all(got[k].tobytes() == want[k].tobytes() for k in want)
    rc, _ = _run(["model", "export", pt, str(tmp_path / "again.pt"), "--format", "torchscript"], caplog)
    assert rc == 0 and sorted(torch.jit.load(str(tmp_path / "again.pt")).state_dict()) == sorted(script.state_dict())


def test_checkpoint_refusals(trained_dir, tmp_path, caplog):
    from remora_amd.__main__ import main
    from remora_amd.train_model import save_model

    with pytest.raises(RemoraError, match=r"^Checkpoint path is not a file \(.*nothing\.checkpoint\)$"):
        _run(["model", "inspect", str(tmp_path / "nothing.checkpoint")], caplog)
    assert main(["model", "export", str(tmp_path / "nothing.checkpoint"), str(tmp_path / "o")]) == 1  # a message and status 1, no traceback
    data = _ckpt_save_data()
    torch.save({**data, "state_dict": None}, str(tmp_path / "stateless.checkpoint"))
    for verb in (["inspect"], ["export", str(tmp_path / "o")]):
        argv = ["model", verb[0], str(tmp_path / "stateless.checkpoint")] + verb[1:]
        with pytest.raises(RemoraError, match=r"^Model state not saved in checkpoint\.$"):
            _run(argv, caplog)
    (tmp_path / "junk.checkpoint").write_bytes(b"\x00" * 64)
    with pytest.raises(RemoraError, match="neither a TorchScript model nor a training checkpoint"):
        _run(["model", "inspect", str(tmp_path / "junk.checkpoint")], caplog)
    # --model-path is read, never run: a file that would leave a mark if executed, and one of the other architecture
    lstm_arch = tmp_path / "lstm_arch.py"
    marker = tmp_path / "executed"
    layers = ["sig_conv1", "sig_conv2", "sig_conv3", "seq_conv1", "seq_conv2", "merge_conv1", "lstm1", "lstm2", "fc"]
    lstm_arch.write_text(f"open({str(marker)!r}, 'w').close()\nclass network:\n    def __init__(self):\n"
                         + "".join(f"        self.{n} = None\n" for n in layers))
    conv_arch = tmp_path / "conv_arch.py"
    conv_arch.write_text("class network:\n    def __init__(self):\n" + "".join(
        f"        self.{n} = None\n" for n in layers[:5] + ["seq_conv3", "merge_conv1", "merge_conv2", "merge_conv3", "merge_conv4", "fc"]))
    for name in ("model_best.checkpoint", "model_best.pt"):
        rc, _ = _run(["model", "inspect", str(trained_dir / name), "--model-path", str(lstm_arch)], caplog)
        assert rc == 0 and not marker.exists()
        with pytest.raises(RemoraError, match="conv_only network, .* conv_lstm network"):
            _run(["model", "export", str(trained_dir / name), str(tmp_path / "o"), "--model-path", str(conv_arch)], caplog)
    assert not os.path.exists(tmp_path / "o")


def test_the_verbs_create_no_engine(trained_dir, tmp_path, caplog, monkeypatch):
    from remora_amd import engine

    def refuse(*a, **k):
        raise AssertionError("an engine was asked for")

    monkeypatch.setattr(engine, "get_engine", refuse)
    monkeypatch.setattr(engine.Engine, "__init__", refuse)
    assert _run(["model", "inspect", str(trained_dir / "model_best.pt")], caplog)[0] == 0
    assert _run(["model", "export", str(trained_dir / "model_best.checkpoint"), str(tmp_path / "d")], caplog)[0] == 0


# ---- 5. the engine's fold on a folded model ------------------------------------------------------------------------------------
def test_the_engines_fold_returns_folded_weights_bit_for_bit(tmp_path):
    """tests/c/identity_fold.cpp: rmr::fold (what rmr_model_create runs) with the statistics the directory reader hands it -
    gamma 1, beta 0, mean 0, var float32(1 - 1e-5) - on 44 116 weights and biases: random values over 81 binades, +-0, the
    neighbours of every power of two, the largest finite values and denormals.  Every one comes back with its bits."""
    clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    assert os.path.exists(clang), clang
    csrc = os.path.join(ROOT, "remora_amd", "csrc")
    exe = str(tmp_path / "identity_fold")
    cc = subprocess.run([clang, "-O3", "-std=c++17", "-Wall", "-I", csrc, os.path.join(ROOT, "tests", "c", "identity_fold.cpp"),
                         os.path.join(csrc, "rmr_pack.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr
    assert run.stdout.strip() == "identity_fold 44116 0"
