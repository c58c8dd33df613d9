"""Model loading for the hot path — drop-in for the load side of `remora.model_util`
(src/remora/model_util.py): load_model :566-699, load_torchscript_model :532-563,
_raw_load_torchscript_model :468-481, add_derived_metadata :341-448.

The model file format is unchanged: a TorchScript archive whose extra file `meta.txt` is a
JSON dict (:115-176).  torch.jit.load is used only to read the file; the weights go to the
HIP engine (BatchNorm folding and MFMA packing happen inside rmr_model_create) and what is
returned in place of the ScriptModule is a `HipModel`.

The training side of the same module: TrainOpts :77-107, CustomPlusCoolDownScheduler :34-74 and
export_model_torchscript :115-176, for remora_amd.train_model; `scan_model_file` stands in for
_load_python_model (:451-465): the architecture file of `--model` is read, never executed.
"""
import ast
import dataclasses
import datetime
import json
import logging
import os
from os.path import isfile

import numpy as np

from . import RemoraError, constants
from .engine import HipModel, _torch, detect_arch
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
    state, md = _raw_load_torchscript_model(model_filename, device)
    add_derived_metadata(md)
    # arithmetic of the GEMM stages: "fp32" (default, exact fp32 MFMA) or a bf16-MFMA mode
    # ("bf16x6" fp32-class split, "bf16x3", "bf16"); REMORA_HIP_DTYPE overrides the default
    dtype = dtype or os.environ.get("REMORA_HIP_DTYPE", "fp32")
    model = HipModel(state, md["chunk_len"], device=device, dtype=dtype)
    if model.kmer_len != md["kmer_len"]:
        raise RemoraError(f"model weights expect kmer_len {model.kmer_len}, metadata says {md['kmer_len']}")
    _record_winograd(model, md, os.path.basename(str(model_filename)))
    return model.eval(), md


def load_model(model_filename=None, *, pore=None, basecall_model_type=None, basecall_model_version=None,
               modified_bases=None, remora_model_type=None, remora_model_version=None, device=None,
               quiet=True, eval_only=False):
    """Same signature as remora.model_util.load_model (:566-578).  Returns
    (HipModel, model_metadata).  Pretrained-model lookup by pore/basecaller needs a network
    download in the reference (:684-695); here it raises RemoraError unless a file is given."""
    if model_filename is not None:
        if not isfile(model_filename):
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
