"""Model loading for the hot path — drop-in for the load side of `remora.model_util`
(src/remora/model_util.py): load_model :566-699, load_torchscript_model :532-563,
_raw_load_torchscript_model :468-481, add_derived_metadata :341-448.

The model file format is unchanged: a TorchScript archive whose extra file `meta.txt` is a
JSON dict (:115-176).  torch.jit.load is used only to read the file; the weights go to the
HIP engine (BatchNorm folding and MFMA packing happen inside rmr_model_create) and what is
returned in place of the ScriptModule is a `HipModel`.

A dorado-format model directory (`config.toml` plus one `*.tensor` file per parameter, the form export_model_dorado :179-309
writes) is the second model format: `load_model` takes the directory, `export_model_dorado` writes it.

The training side of the same module: TrainOpts :77-107, CustomPlusCoolDownScheduler :34-74 and
export_model_torchscript :115-176, for remora_amd.train_model; `scan_model_file` stands in for
_load_python_model (:317-324): the architecture file of `--model` is read, never executed.
"""
import ast
import dataclasses
import datetime
import json
import logging
import os
from os.path import isfile

import numpy as np

from . import RemoraError, constants, toml_lite
from .engine import _CONV_ORDER, HipModel, _torch, detect_arch
from .refine_signal_map import SigMapRefiner

LOGGER = logging.getLogger("Remora")


def winograd_guard_message(model, name):
    """The one line said about a model whose load-time probe took the fp32 Winograd kernels out of use (None otherwise)."""
    rec = model.numerics
    if not rec["checked"] or rec["winograd"]:
        return None
    return (f"model {name}: fp32 Winograd kernels off, direct forms in use (probe of {rec['probe_chunks']} chunks: "
            f"max_abs_diff {rec['max_abs_diff']:.3g} against tol {rec['tol']:.3g}, {rec['nonfinite']} non-finite logits)")


def _record_winograd(model, md, name):
    """metadata["winograd"] = "winograd" / "direct" / "n/a"; one INFO line when the guard tripped."""
    md["winograd"] = model.winograd_form
    msg = winograd_guard_message(model, name)
    if msg is not None:
        LOGGER.info(msg)


def add_derived_metadata(md):
    """Expand the raw `meta.txt` dict the way the reference does (:341-448)."""
    md.setdefault("reverse_signal", False)
    md.setdefault("pa_scaling", None)
    if md["mod_bases"] == "None":
        md["mod_bases"] = None
        md["mod_long_names"] = None
    else:
        md["mod_long_names"] = [md[f"mod_long_names_{i}"] for i in range(len(md["mod_bases"]))]
    if "kmer_context_bases" not in md:
        md["kmer_context_bases"] = (int(md["kmer_context_bases_0"]), int(md["kmer_context_bases_1"]))
    md["kmer_len"] = sum(md["kmer_context_bases"]) + 1
    if "chunk_context" not in md:
        md["chunk_context"] = (int(md["chunk_context_0"]), int(md["chunk_context_1"]))
    md["chunk_len"] = sum(md["chunk_context"])
    if "num_motifs" not in md:
        md["motifs"] = [(md["motif"], int(md["motif_offset"]))]
        md["motif_offset"] = int(md["motif_offset"])
    else:
        md["motifs"] = [(md[f"motif_{i}"], int(md[f"motif_offset_{i}"])) for i in range(int(md["num_motifs"]))]
    md["can_base"] = md["motifs"][0][0][md["motifs"][0][1]]
    md["motif"] = md["motifs"][0] if len(md["motifs"]) == 1 else (md["can_base"], 0)
    if md["mod_bases"] is not None:
        mod_str = "; ".join(f"{b}={n}" for b, n in zip(md["mod_bases"], md["mod_long_names"]))
        md["alphabet_str"] = f"loaded modified base model to call (alt to {md['can_base']}): {mod_str}"
    if md.get("refine_kmer_levels") is not None:
        levels = np.frombuffer(md["refine_kmer_levels"].encode("cp437"), dtype=np.float32)
        sd_arr = np.frombuffer(md["refine_sd_arr"].encode("cp437"), dtype=np.float32)
        md["sig_map_refiner"] = SigMapRefiner(
            _levels_array=levels, center_idx=int(md["refine_kmer_center_idx"]),
            do_rough_rescale=md["refine_do_rough_rescale"], scale_iters=int(md["refine_scale_iters"]),
            algo=md["refine_algo"], half_bandwidth=int(md["refine_half_bandwidth"]), sd_arr=sd_arr)
    else:
        md["sig_map_refiner"] = SigMapRefiner()
        md["base_start_justify"] = False
        md["offset"] = 0
    for k in [k for k in md if k.startswith("refine_")]:
        del md[k]


def _raw_load_torchscript_model(model_filename, device=None):
    torch = _torch()
    extra = {"meta.txt": ""}
    script = torch.jit.load(model_filename, _extra_files=extra, map_location="cpu")
    md = json.loads(extra["meta.txt"])
    state = {k: v.detach().cpu().numpy() for k, v in script.state_dict().items()
             if not k.endswith("num_batches_tracked")}
    return state, md


def load_torchscript_model(model_filename, device=None, quiet=False, eval_only=False, dtype=None):
    """A model file - or a dorado-format model directory (`read_dorado_model`) - onto the engine."""
    if os.path.isdir(model_filename):
        state, md = read_dorado_model(model_filename)
    else:
        state, md = _raw_load_torchscript_model(model_filename, device)
        add_derived_metadata(md)
    # arithmetic of the GEMM stages: "fp32" (default, exact fp32 MFMA) or a bf16-MFMA mode
    # ("bf16x6" fp32-class split, "bf16x3", "bf16"); REMORA_HIP_DTYPE overrides the default
    dtype = dtype or os.environ.get("REMORA_HIP_DTYPE", "fp32")
    model = HipModel(state, md["chunk_len"], device=device, dtype=dtype)
    if model.kmer_len != md["kmer_len"]:
        raise RemoraError(f"model weights expect kmer_len {model.kmer_len}, metadata says {md['kmer_len']}")
    _record_winograd(model, md, os.path.basename(os.path.normpath(str(model_filename))))
    return model.eval(), md


# ---- dorado-format model directories ------------------------------------------------------------------------------------------
DORADO_CONFIG = "config.toml"
DORADO_MODELS = ("conv_lstm", "conv_only")
_LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
_LEVELS_TENSOR = "refine_kmer_levels"


def _lost_field_defaults():
    """What the directory format does not carry, and the value `read_dorado_model` assumes for each."""
    dflt = SigMapRefiner()
    return {"base_start_justify": False, "modified_base_labels": True, "refine_scale_iters": dflt.scale_iters,
            "refine_algo": dflt.algo, "refine_half_bandwidth": dflt.half_bandwidth, "refine_sd_arr": dflt.sd_arr,
            "model_version": constants.MODEL_VERSION}


def ordered_layers(arch):
    """The layers with weights, BatchNorms aside, in `named_modules` order: creation order in the networks of nets.py."""
    convs = [c for c, _ in _CONV_ORDER[arch]]
    return convs + (["lstm1", "lstm2"] if arch == "conv_lstm" else []) + ["fc"]


def dorado_tensor_names(arch):
    """The `<layer>.<key>` names of the tensor files of an architecture, in the exporter's order."""
    return [f"{layer}.{key}" for layer in ordered_layers(arch)
            for key in (_LSTM_KEYS if layer.startswith("lstm") else ("weight", "bias"))]


def save_tensor_file(path, array):
    """One `.tensor` file: the TorchScript archive of an empty module with the single parameter "0" (:188-194)."""
    torch = _torch()
    m = torch.nn.Module()
    x = array.detach() if hasattr(array, "detach") else torch.from_numpy(np.ascontiguousarray(array))
    m.register_parameter("0", torch.nn.Parameter(x, requires_grad=False))
    torch.jit.script(m).save(str(path))


def load_tensor_file(path):
    """The single parameter or buffer of a `.tensor` file, whatever its name, as a numpy array."""
    torch = _torch()
    try:
        m = torch.jit.load(str(path), map_location="cpu")
    except RuntimeError as e:
        raise RemoraError(f"{path}: not a TorchScript tensor file ({str(e).splitlines()[0]})")
    vals = list(m.parameters()) + list(m.buffers())
    if len(vals) != 1:
        raise RemoraError(f"{path}: expected one tensor, found {len(vals)}")
    return vals[0].detach().cpu().numpy()


def read_dorado_model(model_dir):
    """`config.toml` and the tensor files of a dorado-format directory -> (state, metadata): the state in torch's names
    with identity BatchNorm statistics beside every (already folded) convolution, the metadata as `add_derived_metadata`
    leaves that of a model file.  No engine and no GPU is touched."""
    model_dir = str(model_dir)
    cfg_path = os.path.join(model_dir, DORADO_CONFIG)
    if not isfile(cfg_path):
        raise RemoraError(f"Remora model directory ({model_dir}) holds no {DORADO_CONFIG}.")
    cfg = toml_lite.load(cfg_path)
    for table in ("general", "modbases"):
        if not isinstance(cfg.get(table), dict):
            raise RemoraError(f"{cfg_path}: no [{table}] table")
    kind = cfg["general"].get("model")
    if kind not in DORADO_MODELS:
        raise RemoraError(f"{cfg_path}: general.model = {kind!r} is not a model type of this engine; supported: "
                          f"{DORADO_MODELS[0]!r} and {DORADO_MODELS[1]!r}")
    names = sorted(f[: -len(".tensor")] for f in os.listdir(model_dir) if f.endswith(".tensor"))
    layers = {n.split(".")[0] for n in names} - {_LEVELS_TENSOR}
    want = dorado_tensor_names(kind)
    try:
        arch = detect_arch(layers)
    except RemoraError:
        missing = [n for n in want if n not in names]
        if missing:
            raise RemoraError(f"{model_dir}: tensor file {missing[0]}.tensor of a {kind} model is missing"
                              + (f" (and {len(missing) - 1} more)" if len(missing) > 1 else ""))
        raise
    if arch != kind:
        raise RemoraError(f"{model_dir}: the tensor files are those of a {arch} model, {DORADO_CONFIG} says general.model = {kind!r}")
    for n in want:
        if n not in names:
            raise RemoraError(f"{model_dir}: tensor file {n}.tensor of a {kind} model is missing")
    state = {n: load_tensor_file(os.path.join(model_dir, n + ".tensor")).astype(np.float32, copy=False) for n in want}
    # the convolutions are folded already and rmr_model_create folds once more: statistics under which its fold returns
    # every weight and bias bit for bit (scale 1 / sqrt(float32(1 - 1e-5) + 1e-5) = 1 + 6.8e-9, under fp32's half ulp)
    for conv, bn in _CONV_ORDER[arch]:
        oc = state[f"{conv}.weight"].shape[0]
        state[f"{bn}.weight"] = np.ones(oc, np.float32)
        state[f"{bn}.bias"] = np.zeros(oc, np.float32)
        state[f"{bn}.running_mean"] = np.zeros(oc, np.float32)
        state[f"{bn}.running_var"] = np.full(oc, np.float32(1 - 1e-5), np.float32)

    mb, refinement = cfg["modbases"], cfg.get("refinement", {})
    lost = _lost_field_defaults()
    try:
        md = {"creation_date": cfg["general"].get("creation_date"),
              "kmer_context_bases": [int(mb["kmer_context_bases_0"]), int(mb["kmer_context_bases_1"])],
              "chunk_context": [int(mb["chunk_context_0"]), int(mb["chunk_context_1"])],
              "modified_base_labels": lost["modified_base_labels"], "mod_bases": mb.get("mod_bases", "None"),
              "reverse_signal": bool(mb.get("reverse_signal", False)), "base_start_justify": lost["base_start_justify"],
              "offset": int(mb.get("offset", 0)), "pa_scaling": mb.get("pa_scaling"),
              "model_params": dict(cfg.get("model_params", {})),
              "motif_0": str(mb["motif"]), "motif_offset_0": str(int(mb["motif_offset"])), "num_motifs": "1",
              "doc_string": "Nanopore Remora model", "model_version": lost["model_version"]}
        if md["mod_bases"] != "None":
            for i in range(len(md["mod_bases"])):
                md[f"mod_long_names_{i}"] = str(mb[f"mod_long_names_{i}"])
    except KeyError as e:
        raise RemoraError(f"{cfg_path}: [modbases] has no {e.args[0]}")
    offset = md["offset"]
    add_derived_metadata(md)  # no level table in `md`: the default refiner, and the offset taken for 0
    md["offset"] = offset
    if refinement.get("refine_do_rough_rescale"):
        if _LEVELS_TENSOR not in names:
            raise RemoraError(f"{model_dir}: refine_do_rough_rescale is set and {_LEVELS_TENSOR}.tensor is missing")
        if "refine_kmer_center_idx" not in refinement:
            raise RemoraError(f"{cfg_path}: refine_do_rough_rescale is set and refine_kmer_center_idx is missing")
        levels = load_tensor_file(os.path.join(model_dir, _LEVELS_TENSOR + ".tensor")).astype(np.float32, copy=False)
        md["sig_map_refiner"] = SigMapRefiner(_levels_array=levels, center_idx=int(refinement["refine_kmer_center_idx"]),
                                              do_rough_rescale=True)
    LOGGER.info(f"model directory {model_dir}: the format does not carry {', '.join(lost)}; defaults assumed")
    return state, md


def refiner_from_checkpoint(ckpt):
    """The SigMapRefiner of a checkpoint: `sig_map_refiner` where metadata of a loaded model file is passed, otherwise built
    from the `refine_*` entries of a training checkpoint (src/remora/parsers.py:1073-1091)."""
    if ckpt.get("sig_map_refiner") is not None:
        return ckpt["sig_map_refiner"]
    if ckpt.get("refine_kmer_levels") is None:
        return SigMapRefiner()
    return SigMapRefiner(_levels_array=np.asarray(ckpt["refine_kmer_levels"]), center_idx=int(ckpt["refine_kmer_center_idx"]),
                         do_rough_rescale=ckpt["refine_do_rough_rescale"], scale_iters=int(ckpt["refine_scale_iters"]),
                         algo=ckpt["refine_algo"], half_bandwidth=int(ckpt["refine_half_bandwidth"]),
                         sd_arr=np.asarray(ckpt["refine_sd_arr"]))


def repr_model_metadata(metadata):
    """One line per attribute, the per-index entries of parsed values left out (:451-465)."""
    skip = ("mod_long_names_", "kmer_context_bases_", "chunk_context_", "motif_")
    return "\n".join(f"  {k: >20} : {v}" for k, v in metadata.items() if not any(k.startswith(p) for p in skip))


def load_checkpoint(ckpt_path, model_path=None):
    """A training checkpoint as `train_model.save_model` writes it (continue_from_checkpoint :327-338).  `model_path` (default:
    the checkpoint's own, where that file still exists) is scanned for its layer names and never executed; it has to name
    the architecture the checkpoint's state holds."""
    torch = _torch()
    if not isfile(ckpt_path):
        raise RemoraError(f"Checkpoint path is not a file ({ckpt_path})")
    import pickle

    try:
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=False)
    except (pickle.UnpicklingError, RuntimeError, EOFError, ValueError) as e:
        raise RemoraError(f"{ckpt_path} is neither a TorchScript model nor a training checkpoint ({str(e).splitlines()[0]})")
    if not isinstance(ckpt, dict) or "state_dict" not in ckpt:
        raise RemoraError(f"{ckpt_path} is no training checkpoint: no state_dict entry")
    if ckpt["state_dict"] is None:
        raise RemoraError("Model state not saved in checkpoint.")
    arch = detect_arch({k.split(".")[0] for k in ckpt["state_dict"]})
    if model_path is None and ckpt.get("model_path") is not None and isfile(ckpt["model_path"]):
        model_path = ckpt["model_path"]
    if model_path is not None:
        if not isfile(model_path):
            raise RemoraError(f"--model-path {model_path} is not a file")
        scanned = scan_model_file(model_path)
        if scanned != arch:
            raise RemoraError(f"--model-path {model_path} assigns the layers of a {scanned} network, the checkpoint's state is "
                              f"that of a {arch} network")
    return ckpt


def load_model(model_filename=None, *, pore=None, basecall_model_type=None, basecall_model_version=None,
               modified_bases=None, remora_model_type=None, remora_model_version=None, device=None,
               quiet=True, eval_only=False):
    """Same signature as remora.model_util.load_model (:566-578).  Returns
    (HipModel, model_metadata).  `model_filename` is a TorchScript model file or a dorado-format model directory.
    Pretrained-model lookup by pore/basecaller needs a network
    download in the reference (:684-695); here it raises RemoraError unless a file is given."""
    if model_filename is not None:
        if os.path.isdir(model_filename):  # a dorado-format model directory
            if not isfile(os.path.join(model_filename, DORADO_CONFIG)):
                raise RemoraError(f"Remora model directory ({model_filename}) holds no {DORADO_CONFIG}.")
        elif not isfile(model_filename):
            raise RemoraError(f"Remora model file ({model_filename}) not found.")
        try:
            return load_torchscript_model(model_filename, device, quiet=quiet, eval_only=eval_only)
        except (AttributeError, RuntimeError, KeyError, json.JSONDecodeError):
            raise RemoraError("Failed loading torchscript model.")
    if pore is None:
        raise RemoraError("Must specify a pore.")
    raise RemoraError(
        f"load_model(pore={pore!r}, basecall_model_type={basecall_model_type!r}, ..., modified_bases={modified_bases!r}): the "
        "reference resolves these through its pretrained-model registry and downloads the file "
        "(remora.model_util.load_model, src/remora/model_util.py:592-699 -> get_pretrained_models / ModelDownload); that "
        "registry is outside this engine's scope - pass model_filename= (the TorchScript .pt with meta.txt that "
        "`remora model download` or the reference's load_model caches under its models directory)")


def model_from_state(state, model_metadata, device=None, engine=None, dtype="fp32"):
    """HipModel straight from a state_dict-like {name: array} (numpy or torch) — the entry point
    for callers that already hold the weights.  The form the fp32 kernels run it in goes into `model_metadata["winograd"]`."""
    st = {}
    for k, v in state.items():
        if k.endswith("num_batches_tracked"):
            continue
        st[k] = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    model = HipModel(st, int(sum(model_metadata["chunk_context"])), device=device, engine=engine, dtype=dtype)
    _record_winograd(model, model_metadata, f"{model.arch} size {model.size} (from state)")
    return model


# ---- training options (src/remora/model_util.py:34-107) ----------------------------------------------------------------------
TYPE_CONVERTERS = {"str": str, "int": int, "float": float}


def _typed_kwargs(triples):
    """((name, value, type name), ...) of --optimizer-kwargs / --lr-scheduler-kwargs -> {name: converted value}."""
    out = {}
    for name, value, type_name in triples:
        if type_name not in TYPE_CONVERTERS:
            raise RemoraError(f"argument type must be one of {sorted(TYPE_CONVERTERS)}, got {type_name!r} for {name}")
        out[name] = TYPE_CONVERTERS[type_name](value)
    return out


class CustomPlusCoolDownScheduler:
    """Any torch.optim.lr_scheduler class for the first `epochs` - 1 steps, a constant cool-down rate afterwards.  `opt` is a
    torch optimiser; here it is a dummy over one parameter whose only job is to carry the learning rate, read once per epoch
    (the AdamW arithmetic runs in rmr_trainer_adamw_step)."""

    def __init__(self, opt, initial_lr, lr_scheduler_str, lr_scheduler_kwargs, epochs, cool_down_epochs, cool_down_lr):
        torch = _torch()
        self.opt, self.initial_lr = opt, initial_lr
        self.num_epochs, self.num_cool_down_epochs, self.cool_down_lr = epochs, cool_down_epochs, cool_down_lr
        self.total_epochs = epochs + cool_down_epochs
        self.last_epoch = -1
        if not hasattr(torch.optim.lr_scheduler, lr_scheduler_str):
            raise RemoraError(f"torch.optim.lr_scheduler has no {lr_scheduler_str}")
        self.custom_scheduler = getattr(torch.optim.lr_scheduler, lr_scheduler_str)(opt, **_typed_kwargs(lr_scheduler_kwargs))

    def _cooling(self):
        return self.last_epoch >= self.num_epochs - 1

    def get_last_lr(self):
        return [self.cool_down_lr for _ in self.opt.param_groups] if self._cooling() else self.custom_scheduler.get_last_lr()

    def step(self):
        self.last_epoch += 1
        if not self._cooling():
            import warnings

            with warnings.catch_warnings():  # the dummy optimiser never steps: torch's order-of-calls advice does not apply
                warnings.filterwarnings("ignore", message="Detected call of `lr_scheduler.step\\(\\)` before")
                return self.custom_scheduler.step()
        for group in self.opt.param_groups:
            group["lr"] = self.cool_down_lr

    @property
    def lr(self):
        """The rate the next epoch's steps run at: what the optimiser's (only) parameter group holds."""
        return float(self.opt.param_groups[0]["lr"])


@dataclasses.dataclass
class TrainOpts:
    epochs: int = constants.DEFAULT_EPOCHS
    early_stopping: int = constants.DEFAULT_EARLY_STOPPING
    optimizer_str: str = constants.DEFAULT_OPTIMIZER
    opt_kwargs: tuple = constants.DEFAULT_OPT_VALUES
    learning_rate: float = constants.DEFAULT_LR
    lr_scheduler_str: str = constants.DEFAULT_SCHEDULER
    lr_scheduler_kwargs: tuple = constants.DEFAULT_SCH_VALUES
    lr_cool_down_epochs: int = constants.DEFAULT_SCH_COOL_DOWN_EPOCHS
    lr_cool_down_lr: float = constants.DEFAULT_SCH_COOL_DOWN_LR

    ADAMW_KWARGS = ("lr", "weight_decay", "eps")

    def optimizer_kwargs(self):
        """The AdamW arguments of --optimizer-kwargs.  As in the reference (:89-96) --lr is NOT among them: the rate is
        AdamW's default 1e-3 unless `--optimizer-kwargs lr VALUE float` is given."""
        if self.optimizer_str != "AdamW":
            raise RemoraError(f"--optimizer {self.optimizer_str}: the HIP trainer implements AdamW only")
        kw = _typed_kwargs(self.opt_kwargs)
        unknown = sorted(set(kw) - set(self.ADAMW_KWARGS))
        if unknown:
            raise RemoraError(f"--optimizer-kwargs {unknown}: the HIP trainer takes {list(self.ADAMW_KWARGS)}")
        return kw

    def load_optimizer(self, model=None):
        """A torch AdamW over one dummy parameter with the run's arguments: the scheduler's handle on the learning rate."""
        torch = _torch()
        return torch.optim.AdamW([torch.zeros(1, requires_grad=True)], **self.optimizer_kwargs())

    def load_scheduler(self, opt):
        return CustomPlusCoolDownScheduler(opt, self.learning_rate, self.lr_scheduler_str, self.lr_scheduler_kwargs, epochs=self.epochs,
                                           cool_down_epochs=self.lr_cool_down_epochs, cool_down_lr=self.lr_cool_down_lr)


def scan_model_file(model_path):
    """The architecture of a `--model` file ("conv_lstm" / "conv_only") from the layer names its classes assign to `self`
    (detect_arch's rule).  The file is parsed, never imported or executed."""
    with open(model_path) as fh:
        try:
            tree = ast.parse(fh.read(), filename=str(model_path))
        except SyntaxError as e:
            raise RemoraError(f"cannot parse model file {model_path}: {e}")
    names = set()
    for node in ast.walk(tree):
        targets = node.targets if isinstance(node, ast.Assign) else [node.target] if isinstance(node, (ast.AnnAssign, ast.AugAssign)) else []
        for tgt in targets:
            for t in (tgt.elts if isinstance(tgt, (ast.Tuple, ast.List)) else [tgt]):
                if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id == "self":
                    names.add(t.attr)
    return detect_arch(names)


# ---- export (src/remora/model_util.py:115-176) ---------------------------------------------------------------------------------
_META_KEYS = ("kmer_context_bases", "chunk_context", "modified_base_labels", "mod_bases", "reverse_signal", "refine_kmer_center_idx",
              "refine_do_rough_rescale", "refine_scale_iters", "refine_algo", "refine_half_bandwidth", "base_start_justify", "offset",
              "pa_scaling", "model_params")


def export_model_torchscript(ckpt, state, save_filename):
    """The model file of the reference: a TorchScript archive of the network (remora_amd.nets, eval mode) holding `state`
    (a state_dict; default: ckpt["state_dict"]) with the extra file meta.txt built from the checkpoint's entries.  Loads through
    `load_model` here and through torch.jit.load anywhere."""
    torch = _torch()
    from . import nets

    def plain(v):  # JSON has no numpy scalars or arrays
        if isinstance(v, np.ndarray):
            return v.tolist()
        if isinstance(v, np.generic):
            return v.item()
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        return v

    script = torch.jit.script(nets.from_state(ckpt["state_dict"] if state is None else state))
    meta = {"creation_date": datetime.datetime.now().strftime("%m/%d/%Y, %H:%M:%S")}
    for key in _META_KEYS:
        meta[key] = plain(ckpt[key])
    if ckpt["mod_bases"] is not None:
        for i, name in enumerate(ckpt["mod_long_names"]):
            meta[f"mod_long_names_{i}"] = str(name)
    for i, (motif, offset) in enumerate(ckpt["motifs"]):
        meta[f"motif_{i}"], meta[f"motif_offset_{i}"] = str(motif), str(offset)
    meta["num_motifs"] = str(len(ckpt["motifs"]))
    for key in ("refine_kmer_levels", "refine_sd_arr"):  # float32 bytes carried as cp437 text
        meta[key] = None if ckpt[key] is None else np.asarray(ckpt[key]).astype(np.float32).tobytes().decode("cp437")
    meta["doc_string"] = "Nanopore Remora model"
    meta["model_version"] = ckpt.get("model_version", 0)
    torch.jit.save(script, save_filename, _extra_files={"meta.txt": json.dumps(meta, indent=4)})


def export_model_dorado(ckpt, state, save_dir):
    """The dorado-format directory of the reference (:179-309): every convolution folded with its BatchNorm by torch's
    fuse_conv_bn_eval in fp32, one `<layer>.<key>.tensor` file per entry of each layer's state_dict, `config.toml` with the
    tables general, model_params, modbases and refinement.  `state` as in export_model_torchscript.  The refiner comes from
    `refiner_from_checkpoint`, so a training checkpoint exports as a loaded model file does."""
    torch = _torch()
    from torch.nn.utils.fusion import fuse_conv_bn_eval

    from . import nets

    if len(ckpt["motifs"]) > 1:  # before anything is written
        raise RemoraError("Dorado only supports models with a single motif")
    save_dir = os.path.expanduser(str(save_dir))
    if os.path.exists(save_dir):
        LOGGER.info(f'Directory "{save_dir}" already exists. Exported files will be overwritten.')
    os.makedirs(save_dir, exist_ok=True)

    net = nets.from_state(ckpt["state_dict"] if state is None else state)  # eval mode
    arch = detect_arch({name for name, _ in net.named_children()})
    conv_to_bn = dict(_CONV_ORDER[arch])
    layer_names = []
    for name, module in net.named_modules():
        if name == "" or "bn" in name or "drop" in name:
            continue
        if name in conv_to_bn:
            fused = fuse_conv_bn_eval(module, getattr(net, conv_to_bn[name]))
            module.weight, module.bias = fused.weight, fused.bias
        for k, v in module.state_dict().items():
            save_tensor_file(os.path.join(save_dir, f"{name}.{k}.tensor"), v)
        layer_names.append(name)
    if layer_names != ordered_layers(arch):
        raise RemoraError(f"export walked the layers {layer_names}, expected {ordered_layers(arch)}")

    general = {"creation_date": datetime.datetime.now().strftime("%m/%d/%Y, %H:%M:%S"), "model": arch}
    refiner = refiner_from_checkpoint(ckpt)
    refinement = {"refine_do_rough_rescale": int(refiner.do_rough_rescale)}  # dorado reads an int here
    if refiner.do_rough_rescale:
        refinement["refine_kmer_center_idx"] = int(refiner.center_idx)
        save_tensor_file(os.path.join(save_dir, _LEVELS_TENSOR + ".tensor"), np.asarray(refiner._levels_array).astype(np.float32))
    modbases = {key: ckpt[key] for key in ("mod_bases", "offset", "reverse_signal", "pa_scaling")}
    if ckpt["mod_bases"] is not None:
        for i in range(len(ckpt["mod_bases"])):
            modbases[f"mod_long_names_{i}"] = str(ckpt["mod_long_names"][i])
    for key in ("chunk_context", "kmer_context_bases"):
        for i in range(2):
            modbases[f"{key}_{i}"] = int(ckpt[key][i])
    motif, motif_offset = ckpt["motifs"][0]
    modbases["motif"], modbases["motif_offset"] = str(motif), int(motif_offset)
    toml_lite.dump({"general": general, "model_params": dict(ckpt["model_params"]), "modbases": modbases, "refinement": refinement},
                   os.path.join(save_dir, DORADO_CONFIG))

    # what the directory does not carry: said once per field whose value the loader's default would change
    held = {"refine_scale_iters": refiner.scale_iters, "refine_algo": refiner.algo, "refine_half_bandwidth": refiner.half_bandwidth,
            "refine_sd_arr": refiner.sd_arr}
    for field, default in _lost_field_defaults().items():
        if field in held:
            value = held[field]
        elif field in ckpt:
            value = ckpt[field]
        else:
            continue
        same = np.array_equal(np.asarray(value), np.asarray(default)) if field == "refine_sd_arr" else value == default
        if not same:
            LOGGER.warning(f"dorado format does not carry {field} ({value!r}): a model loaded from {save_dir} takes {default!r}")
