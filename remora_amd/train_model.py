"""`remora model train` on the HIP engine — drop-in for src/remora/train_model.py.

`Trainer` is the model + optimiser pair of the reference's loop (train_model.py:333-360, :470-503) over rmr_trainer_*:
the forward pass with BatchNorm in train mode, the loss, the backward pass and AdamW all run on the device; torch draws
the initial weights on the CPU (remora_amd/nets.py) and is the container of `state_dict()` / checkpoints.
"""
import atexit
import ctypes
import json
import logging
import os
from collections import OrderedDict
from itertools import islice
from shutil import copyfile

import numpy as np

from . import RemoraError, constants
from . import _lib as L
from .engine import _torch, detect_arch, get_engine, state_to_blob

LOGGER = logging.getLogger("Remora")
BREACH_THRESHOLD = 0.8
REGRESSION_THRESHOLD = 0.7
MAD_TO_SD = 1.4826  # mad(N(0, sigma^2)) * 1.4826 = sigma

ADAMW_DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)


class Trainer:
    """One ConvLSTM_w_ref network in training on one GPU: parameters, running statistics, gradients and AdamW moments live
    in flat device buffers (the order of `engine.state_to_blob`).  fp32; `size` a multiple of 16 from 16 to 256.

    Without `state` the initial weights are what the reference draws for `seed` (`nets.build`)."""

    def __init__(self, size, kmer_len, num_out, chunk_len, max_batch, state=None, seed=None, device=None, **opt_kwargs):
        from . import nets

        self.size, self.kmer_len, self.num_out = int(size), int(kmer_len), int(num_out)
        self.chunk_len, self.max_batch = int(chunk_len), int(max_batch)
        unknown = set(opt_kwargs) - set(ADAMW_DEFAULTS)
        if unknown:
            raise RemoraError(f"unknown AdamW arguments {sorted(unknown)}")
        self.opt = dict(ADAMW_DEFAULTS, **opt_kwargs)
        if state is None:
            state = nets.build(self.size, self.kmer_len, self.num_out, seed=seed).state_dict()
        state = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in state.items()}
        arch = detect_arch({k.split(".")[0] for k in state})
        if arch == "conv_lstm":
            _, s_size, s_kmer, s_out, blob = state_to_blob(state)
            if (s_size, s_kmer, s_out) != (self.size, self.kmer_len, self.num_out):
                raise RemoraError(f"state is size {s_size}, kmer_len {s_kmer}, num_out {s_out}; the trainer was asked for "
                                  f"{self.size}, {self.kmer_len}, {self.num_out}")
        else:
            blob = np.zeros(1, np.float32)  # refused by name below
        self.engine = get_engine(device)
        self._lib = lib = L.lib()
        desc = L.ModelDesc(L.ARCH_CONV_LSTM if arch == "conv_lstm" else L.ARCH_CONV_ONLY, self.size, self.kmer_len, self.num_out,
                           self.chunk_len, 0)
        blob = np.ascontiguousarray(blob, np.float32)
        h = ctypes.c_void_p()
        L.check(lib.rmr_trainer_create(self.engine.handle, ctypes.byref(desc), blob.ctypes.data, blob.size, self.max_batch, ctypes.byref(h)))
        self._h = h
        self.n_floats = int(blob.size)
        n = ctypes.c_int(0)
        L.check(lib.rmr_trainer_tensor_layout(h, 0, None, None, None, None, ctypes.byref(n)))
        names = ctypes.create_string_buffer(n.value * L.TRAIN_NAME_LEN)
        off, size_, par = np.zeros(n.value, np.int64), np.zeros(n.value, np.int64), np.zeros(n.value, np.int32)
        L.check(lib.rmr_trainer_tensor_layout(h, n.value, names, off.ctypes.data, size_.ctypes.data, par.ctypes.data, ctypes.byref(n)))
        shapes = {k: tuple(v.shape) for k, v in state.items()}
        # (name, offset, size, shape, is_param) of every tensor of the flat buffers, in their order
        self.layout = []
        for i in range(n.value):
            name = names.raw[i * L.TRAIN_NAME_LEN:(i + 1) * L.TRAIN_NAME_LEN].split(b"\0")[0].decode()
            self.layout.append((name, int(off[i]), int(size_[i]), shapes[name], bool(par[i])))
        self.param_names = [t[0] for t in self.layout if t[4]]  # named_parameters order
        if "sig_bn1.num_batches_tracked" in state:
            self._set_counters(batches=int(state["sig_bn1.num_batches_tracked"]))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._lib.rmr_trainer_destroy(h)
            except Exception:
                pass

    # ---- flat buffers ----
    def _read(self, which, n=None):
        out = np.empty(self.n_floats if n is None else n, np.float32)
        L.check(self._lib.rmr_trainer_read(self._h, which, out.ctypes.data, out.size))
        return out

    def _write(self, which, arr):
        arr = np.ascontiguousarray(arr, np.float32)
        L.check(self._lib.rmr_trainer_write(self._h, which, arr.ctypes.data, arr.size))

    def _counters(self):
        c = self._read(L.TRAIN_COUNTERS, 3)
        return int(c[0]), int(c[1]), float(c[2])

    def _set_counters(self, steps=None, batches=None):
        s, b, _ = self._counters()
        self._write(L.TRAIN_COUNTERS, np.array([s if steps is None else steps, b if batches is None else batches, 0], np.float32))

    @property
    def optimizer_steps(self):
        return self._counters()[0]

    @property
    def workspace_bytes_per_chunk(self):
        return self._counters()[2]

    def _split(self, flat, params_only):
        return OrderedDict((name, flat[off:off + size].reshape(shape).copy()) for name, off, size, shape, par in self.layout
                           if par or not params_only)

    def _join(self, tensors, into):
        for name, off, size, shape, par in self.layout:
            if name in tensors:
                v = tensors[name]
                v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
                if tuple(v.shape) != shape:
                    raise RemoraError(f"{name}: shape {tuple(v.shape)}, expected {shape}")
                into[off:off + size] = v.astype(np.float32).ravel()
        return into

    # ---- the step ----
    def forward_backward(self, sigs, enc_kmers, labels, mask=None, return_logits=False):
        """sigs f32[n,1,L], enc_kmers f32[n,4K,L], labels i64[n], mask bool[n] or None (rows with False leave the loss but
        still take part in BatchNorm): fills the gradients, moves the running statistics, returns the mean cross-entropy
        (and the logits).  numpy / CPU tensors are staged; CUDA tensors are read in place.

        A label outside 0..num_out-1 in a row of the loss raises RemoraError ("label ... outside 0..num_out-1") and leaves the
        gradients, the running statistics and num_batches_tracked as they were.  Host labels are checked before any launch.
        Device labels are checked by the step's first kernel, before the BatchNorm launches: those kernels hold their stores to
        the running statistics and the gradients, and the error is raised once the loss has been read - no synchronisation is
        added for it."""
        torch = _torch()
        on_dev = isinstance(sigs, torch.Tensor) and sigs.is_cuda
        want = [(sigs, np.float32, torch.float32), (enc_kmers, np.float32, torch.float32), (labels, np.int64, torch.int64)]
        if mask is not None:
            want.append((mask, np.uint8, torch.uint8))
        bufs = []
        for x, npd, tod in want:
            if on_dev:
                if not (isinstance(x, torch.Tensor) and x.is_cuda):
                    raise RemoraError("all training inputs must share the signal's residency")
                bufs.append(x.to(tod).contiguous())
            else:
                if isinstance(x, torch.Tensor):
                    x = x.cpu().numpy()
                bufs.append(np.ascontiguousarray(x, npd))
        n = int(bufs[0].shape[0])
        if tuple(bufs[0].shape) != (n, 1, self.chunk_len) or tuple(bufs[1].shape) != (n, 4 * self.kmer_len, self.chunk_len) or \
                tuple(bufs[2].shape) != (n,) or (mask is not None and tuple(bufs[3].shape) != (n,)):
            raise RemoraError(f"expected sigs [n,1,{self.chunk_len}], enc_kmers [n,{4 * self.kmer_len},{self.chunk_len}], labels [n]; got "
                              f"{[tuple(b.shape) for b in bufs]}")
        ptr = (lambda b: b.data_ptr()) if on_dev else (lambda b: b.ctypes.data)
        logits = None
        if return_logits:
            logits = (torch.empty((n, self.num_out), dtype=torch.float32, device=bufs[0].device) if on_dev
                      else np.empty((n, self.num_out), np.float32))
        loss = ctypes.c_float(0)
        L.check(self._lib.rmr_trainer_forward_backward(
            self._h, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]) if mask is not None else None, n, ctypes.byref(loss),
            ptr(logits) if return_logits else None, L.MEM_DEVICE if on_dev else L.MEM_HOST))
        return (loss.value, logits) if return_logits else loss.value

    def grad_absmax(self):
        """max |grad| per parameter tensor, named_parameters order (apply_clipping's grad_maxs, train_model.py:118-123)."""
        out = np.empty(len(self.param_names), np.float32)
        L.check(self._lib.rmr_trainer_grad_absmax(self._h, out.ctypes.data))
        return out

    def optimizer_step(self, lr=None, clip=None):
        """One AdamW step on the current gradients; `clip`: per-tensor thresholds (named_parameters order) the gradients are
        clamped to by value first, or None."""
        o = self.opt
        c = None
        if clip is not None:
            c = np.ascontiguousarray(clip, np.float32)
            if c.shape != (len(self.param_names),):
                raise RemoraError(f"clip needs {len(self.param_names)} thresholds, got shape {c.shape}")
        L.check(self._lib.rmr_trainer_adamw_step(self._h, float(o["lr"] if lr is None else lr), float(o["betas"][0]), float(o["betas"][1]),
                                                 float(o["eps"]), float(o["weight_decay"]), c.ctypes.data if c is not None else None))

    def step(self, sigs, enc_kmers, labels, mask=None, lr=None, clip=None):
        """forward, backward and one AdamW step; returns the batch's loss (before the step)."""
        loss = self.forward_backward(sigs, enc_kmers, labels, mask)
        self.optimizer_step(lr=lr, clip=clip)
        return loss

    # ---- state ----
    def grads(self):
        """{parameter name: gradient array} of the last forward_backward."""
        return self._split(self._read(L.TRAIN_GRADS), params_only=True)

    def state_dict(self):
        """torch names and order, CPU tensors, num_batches_tracked included: loads into the reference's module strict=True."""
        torch = _torch()
        flat = self._split(self._read(L.TRAIN_PARAMS), params_only=False)
        nbt = self._counters()[1]
        out = OrderedDict()
        for name, arr in flat.items():
            out[name] = torch.from_numpy(arr)
            if name.endswith("running_var"):
                out[name[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(nbt, dtype=torch.int64)
        return out

    def load_state_dict(self, state):
        missing = [t[0] for t in self.layout if t[0] not in state]
        if missing:
            raise RemoraError(f"state lacks {missing}")
        self._write(L.TRAIN_PARAMS, self._join(state, np.zeros(self.n_floats, np.float32)))
        nbt = state.get("sig_bn1.num_batches_tracked")
        self._set_counters(batches=int(nbt) if nbt is not None else 0)

    def optimizer_state_dict(self):
        """torch.optim.AdamW.state_dict()'s layout: state[i] = {step, exp_avg, exp_avg_sq} for parameter i of named_parameters
        (empty before the first step, as torch's), one param_group."""
        torch = _torch()
        o = self.opt
        group = torch.optim.AdamW([torch.zeros(1) for _ in self.param_names], lr=o["lr"], betas=tuple(o["betas"]), eps=o["eps"],
                                  weight_decay=o["weight_decay"]).state_dict()["param_groups"]
        steps = self.optimizer_steps
        state = {}
        if steps:
            m = self._split(self._read(L.TRAIN_ADAM_M), params_only=True)
            v = self._split(self._read(L.TRAIN_ADAM_V), params_only=True)
            for i, name in enumerate(self.param_names):
                state[i] = {"step": torch.tensor(float(steps)), "exp_avg": torch.from_numpy(m[name]), "exp_avg_sq": torch.from_numpy(v[name])}
        return {"state": state, "param_groups": group}

    def load_optimizer_state_dict(self, sd):
        g = sd["param_groups"][0]
        self.opt = dict(lr=float(g["lr"]), betas=tuple(float(b) for b in g["betas"]), eps=float(g["eps"]), weight_decay=float(g["weight_decay"]))
        m, v = np.zeros(self.n_floats, np.float32), np.zeros(self.n_floats, np.float32)
        steps = 0
        if sd["state"]:
            if sorted(sd["state"]) != list(range(len(self.param_names))):
                raise RemoraError("optimizer state does not cover the network's parameters")
            self._join({name: sd["state"][i]["exp_avg"] for i, name in enumerate(self.param_names)}, m)
            self._join({name: sd["state"][i]["exp_avg_sq"] for i, name in enumerate(self.param_names)}, v)
            steps = int(sd["state"][0]["step"])
        self._write(L.TRAIN_ADAM_M, m)
        self._write(L.TRAIN_ADAM_V, v)
        self._set_counters(steps=steps)

    def eval_model(self, model_metadata=None):
        """A HipModel (inference kernels, BatchNorm folded with the running statistics) of the current state."""
        from .model_util import model_from_state

        md = model_metadata if model_metadata is not None else {"chunk_context": (self.chunk_len // 2, self.chunk_len - self.chunk_len // 2)}
        return model_from_state(self.state_dict(), md, engine=self.engine)


# ---- gradient clipping (src/remora/train_model.py:33-131) ------------------------------------------------------------------
def med_mad(data, factor=MAD_TO_SD, axis=None, keepdims=False):
    """(median, factor x median absolute deviation from the median) of `data` along `axis`."""
    data = np.asarray(data)
    med = np.median(data, axis=axis, keepdims=True)
    mad = factor * np.median(np.abs(data - med), axis=axis, keepdims=True)
    if axis is None:
        return med.ravel()[0], mad.ravel()[0]
    if not keepdims:
        med, mad = med.squeeze(axis), mad.squeeze(axis)
    return med, mad


class RollingMAD:
    """Per-parameter clip thresholds: median + n_mads x MAD of the last `window` gradient maxima; `default_to` until the
    window has been filled once."""

    def __init__(self, nparams, n_mads=0, window=1000, default_to=None):
        self.n_mads, self.default_to = n_mads, default_to
        self._window_data = np.empty((nparams, window), dtype="f4")
        self._curr_iter = 0

    nparams = property(lambda s: s._window_data.shape[0])
    window = property(lambda s: s._window_data.shape[1])

    def update(self, vals):
        if len(vals) != self.nparams:
            raise RemoraError(f"{len(vals)} values for {self.nparams} parameters")
        self._window_data[:, self._curr_iter % self.window] = vals
        self._curr_iter += 1
        if self._curr_iter < self.window:
            return self.default_to
        med, mad = med_mad(self._window_data, axis=1)
        return med + mad * self.n_mads


def high_conf_incorrect_mask(logits, labels, conf_thresh, max_frac_skip):
    """Rows kept in the loss under --high-conf-incorrect-thr-frac (src/remora/train_model.py:477-497): a row leaves when its
    call is wrong with a probability of at least `conf_thresh`; at most floor(batch x max_frac_skip) rows leave (the
    threshold rises to the probability of the first wrong call that has to stay)."""
    logits, labels = np.asarray(logits, np.float32), np.asarray(labels)
    z = logits - logits.max(axis=1, keepdims=True)
    probs = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    call, top = probs.argmax(axis=1), probs.max(axis=1)
    match = call == labels
    max_skip = int(np.floor(len(labels) * max_frac_skip))
    if len(labels) - match.sum() > max_skip:
        wrong = np.sort(top[~match])[::-1]
        conf_thresh = max(conf_thresh, wrong[max_skip])
    return match | (top < conf_thresh)


# ---- the training run (src/remora/train_model.py:134-647) -------------------------------------------------------------------
_RAW = ("signal", "sequence", "sequence_to_signal_mapping", "sequence_lengths", "labels")


def save_model(trainer, ckpt_save_data, out_path, epoch, model_name=constants.BEST_MODEL_FILENAME, as_torchscript=True,
               model_name_torchscript=constants.BEST_TORCHSCRIPT_MODEL_FILENAME):
    from . import model_util

    torch = _torch()
    ckpt_save_data["epoch"] = epoch + 1
    ckpt_save_data["state_dict"] = trainer.state_dict()
    ckpt_save_data["opt"] = trainer.optimizer_state_dict()
    torch.save(ckpt_save_data, os.path.join(out_path, model_name))
    if as_torchscript:
        model_util.export_model_torchscript(ckpt_save_data, None, os.path.join(out_path, model_name_torchscript))


def _load_val_dataset(path, override_metadata, batch_size):
    from .data_chunks import CoreRemoraDataset, RemoraDataset, load_dataset

    paths, props, hashes = load_dataset(path.strip())
    return RemoraDataset([CoreRemoraDataset(p, override_metadata=dict(override_metadata), infinite_iter=False, do_check_super_batches=True)
                          for p in paths], props, hashes, batch_size=batch_size)


def train_model(seed, device, out_path, remora_dataset_path, chunk_context, kmer_context_bases, batch_size, model_path, size, train_opts,
                chunks_per_epoch, num_test_chunks, save_freq, filt_frac, ext_val, ext_val_names, high_conf_incorrect_thr_frac,
                finetune_path, freeze_num_layers, super_batch_size, super_batch_sample_frac, read_batches_from_disk,
                gradient_clip_num_mads):
    """The reference's signature, files and loop.  What differs: the architecture file is copied and scanned, never executed
    (ConvLSTM_w_ref only); the optimiser is AdamW; fine-tuning is refused; validation batches are always read from the
    dataset's files; the network and the optimiser run as rmr_trainer_* on the GPU of `device`."""
    torch = _torch()
    from . import model_util, util, validate
    from .data_chunks import CoreRemoraDataset, RemoraDataset, load_dataset
    from .encoded_kmers import compute_encoded_kmer_batch

    out_path = str(out_path)
    if finetune_path is not None or freeze_num_layers:
        raise RemoraError("--finetune-path / --freeze-num-layers: fine-tuning is not built for the HIP trainer")
    opt_kwargs = train_opts.optimizer_kwargs()  # refuses another optimiser before anything is loaded
    if model_util.scan_model_file(model_path) != "conv_lstm":
        raise RemoraError(f"--model {model_path} assigns the layers of Conv_w_ref: the HIP trainer trains ConvLSTM_w_ref only")
    seed = int(np.random.randint(0, np.iinfo(np.uint32).max, dtype=np.uint32)) if seed is None else int(seed)
    LOGGER.info(f"Seed selected is {seed}")
    np.random.seed(seed)
    if super_batch_size != constants.DEFAULT_SUPER_BATCH_SIZE or super_batch_sample_frac not in (None, constants.DEFAULT_SUPER_BATCH_SAMPLE_FRAC):
        LOGGER.info("--super-batch-size / --super-batch-sample-fraction are handed to the dataset classes and otherwise ignored")
    if read_batches_from_disk:
        LOGGER.info("--read-batches-from-disk is accepted and ignored: validation batches are always read from the dataset's files")

    LOGGER.info("Loading dataset from Remora dataset config")
    override_metadata = {"extra_arrays": {}}
    if kmer_context_bases is not None:
        override_metadata["kmer_context_bases"] = tuple(kmer_context_bases)
    if chunk_context is not None:
        override_metadata["chunk_context"] = tuple(chunk_context)
    paths, props, hashes = load_dataset(remora_dataset_path)
    dataset = RemoraDataset([CoreRemoraDataset(p, override_metadata=dict(override_metadata)) for p in paths], props, hashes,
                            batch_size=batch_size, super_batch_size=super_batch_size, super_batch_sample_frac=super_batch_sample_frac)
    md = dataset.metadata
    with open(os.path.join(out_path, "dataset_config.jsn"), "w") as fh:
        json.dump(dataset.get_config(), fh)
    md.write(os.path.join(out_path, "dataset_metadata.jsn"))
    LOGGER.info(f"Dataset summary:\n{dataset.summary}")

    val_raw = open(os.path.join(out_path, "validation.log"), mode="w", buffering=1)
    atexit.register(val_raw.close)
    val_fp = validate.ValidationLogger(val_raw)
    batch_fp = open(os.path.join(out_path, "batch.log"), "w", buffering=1)
    atexit.register(batch_fp.close)
    batch_fp.write("Iteration\tLoss\tNumberFiltered\n" if high_conf_incorrect_thr_frac is not None else "Iteration\tLoss\n")

    LOGGER.info("Loading model")
    copy_model_path = util.resolve_path(os.path.join(out_path, "model.py"))
    copyfile(model_path, copy_model_path)
    model_params = {"size": size, "kmer_len": md.kmer_len, "num_out": md.num_labels}
    trainer = Trainer(size, md.kmer_len, md.num_labels, sum(md.chunk_context), max_batch=batch_size, seed=seed, device=device, **opt_kwargs)
    rolling_mads, grad_max_threshs = None, None
    if gradient_clip_num_mads is not None:
        rolling_mads = RollingMAD(len(trainer.param_names), gradient_clip_num_mads)
        LOGGER.info(f"Gradients will be clipped (by value) at {rolling_mads.n_mads:3.2f} MADs above the median of the last "
                    f"{rolling_mads.window} gradient maximums.")

    ext_datasets = []
    if ext_val is not None:
        names = ext_val_names if ext_val_names is not None else [f"e_val_{i}" for i in range(len(ext_val))]
        if len(names) != len(ext_val):
            raise RemoraError("--ext-val-names must name every --ext-val dataset")
        for name, path in zip(names, ext_val):
            ds = _load_val_dataset(path, override_metadata, batch_size)
            ds.update_metadata(dataset)
            ext_datasets.append((name, ds))

    LOGGER.info(f"Training optimizer and scheduler settings: {train_opts}")
    scheduler = train_opts.load_scheduler(train_opts.load_optimizer())
    criterion = torch.nn.CrossEntropyLoss()
    trn_ds, val_ds = dataset.train_test_split(num_test_chunks, override_metadata=override_metadata)
    val_ds.super_batch_sample_frac = None
    val_trn_ds = trn_ds.head(num_test_chunks, override_metadata=override_metadata)
    val_trn_ds.super_batch_sample_frac = None
    for ds in (val_ds, val_trn_ds):
        for core in ds.datasets:
            core.do_check_super_batches = True
    LOGGER.info(f"Dataset loaded with labels: {dataset.label_summary}")
    LOGGER.info(f"Train labels: {trn_ds.label_summary}")
    LOGGER.info(f"Held-out validation labels: {val_ds.label_summary}")
    LOGGER.info(f"Training set validation labels: {val_trn_ds.label_summary}")

    eval_md = {"chunk_context": tuple(md.chunk_context)}

    def validate_all(nepoch, niter):
        model = trainer.eval_model(dict(eval_md))
        common = dict(nepoch=nepoch, niter=niter, disable_pbar=True)
        val = val_fp.validate_model(model, md.mod_bases, criterion, val_ds, filt_frac, **common)
        trn = val_fp.validate_model(model, md.mod_bases, criterion, val_trn_ds, filt_frac, "trn", **common)
        ext = [(name, val_fp.validate_model(model, md.mod_bases, criterion, ds, filt_frac, name, **common)) for name, ds in ext_datasets]
        return val, trn, ext

    LOGGER.info("Running initial validation")
    val_metrics, trn_metrics, _ = validate_all(0, 0)
    batches_per_epoch = int(np.ceil(chunks_per_epoch / batch_size))
    epoch_summ = trn_ds.epoch_summary(batches_per_epoch)
    with open(os.path.join(out_path, "epoch_summary.txt"), "w") as fh:
        fh.write(epoch_summ + "\n")
    best_alt_val_accs = {name: 0 for name, _ in ext_datasets}

    ckpt_save_data = {
        "epoch": 0, "state_dict": trainer.state_dict(), "opt": trainer.optimizer_state_dict(), "model_path": copy_model_path,
        "model_params": model_params, "fixed_seq_len_chunks": False, "model_version": constants.MODEL_VERSION,
        "chunk_context": md.chunk_context, "motifs": md.motifs, "num_motifs": md.num_motifs, "reverse_signal": md.reverse_signal,
        "mod_bases": md.mod_bases, "mod_long_names": md.mod_long_names, "modified_base_labels": md.modified_base_labels,
        "kmer_context_bases": md.kmer_context_bases, "base_start_justify": md.base_start_justify, "offset": md.offset,
        "pa_scaling": md.pa_scaling, **md._refiner_dict(),
    }

    LOGGER.info("Start training")
    dev = trainer.engine.torch_device
    kb, ka = md.kmer_context_bases
    trn_iter = trn_ds.iter_numpy_batches(return_arrays=_RAW, copy=True)
    best_val_acc, early_stop_epochs, breached, epoch = 0, 0, False, -1
    for epoch in range(train_opts.epochs):
        lr = scheduler.lr
        for epoch_i, batch in enumerate(islice(trn_iter, batches_per_epoch)):
            sig, seq, smap, lens, labels = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in batch)
            if labels.shape[0] < 2:
                continue
            enc = compute_encoded_kmer_batch(kb, ka, seq, smap, lens, engine=trainer.engine)  # rmr_encode_kmers, on the device
            mask, n_filt = None, 0
            if high_conf_incorrect_thr_frac is not None:
                # the mask is made from this batch's own train-mode logits: one pass for them (state put back), one with the mask
                snapshot, counters = trainer._read(L.TRAIN_PARAMS), trainer._counters()
                _, logits = trainer.forward_backward(sig, enc, labels, return_logits=True)
                trainer._write(L.TRAIN_PARAMS, snapshot)
                trainer._set_counters(batches=counters[1])
                keep = high_conf_incorrect_mask(logits.cpu().numpy(), batch[4], *high_conf_incorrect_thr_frac)
                mask, n_filt = torch.from_numpy(keep.astype(np.uint8)).to(dev), int((~keep).sum())
            loss = trainer.forward_backward(sig, enc, labels, mask=mask)
            grad_maxs = trainer.grad_absmax() if rolling_mads is not None else None
            trainer.optimizer_step(lr=lr, clip=grad_max_threshs)
            if rolling_mads is not None:
                grad_max_threshs = rolling_mads.update(grad_maxs)
            batch_fp.write(f"{epoch * batches_per_epoch + epoch_i}\t{loss:.6f}" + (f"\t{n_filt}\n" if mask is not None else "\n"))

        niter = (epoch + 1) * batches_per_epoch
        val_metrics, trn_metrics, ext_metrics = validate_all(epoch + 1, niter)
        scheduler.step()
        if breached:
            if val_metrics.acc <= REGRESSION_THRESHOLD:
                LOGGER.warning("Remora training unstable")
        elif val_metrics.acc >= BREACH_THRESHOLD:
            breached = True
        if val_metrics.acc > best_val_acc:
            best_val_acc, early_stop_epochs = val_metrics.acc, 0
            save_model(trainer, ckpt_save_data, out_path, epoch)
        else:
            early_stop_epochs += 1
        for name, ms in ext_metrics:
            if ms.acc <= best_alt_val_accs[name]:
                continue
            best_alt_val_accs[name], early_stop_epochs = ms.acc, 0
            save_model(trainer, ckpt_save_data, out_path, epoch, model_name=f"model_ext_val_{name}_best.checkpoint",
                       model_name_torchscript=f"model_ext_val_{name}_best.pt")
        if (epoch + 1) % save_freq == 0:
            save_model(trainer, ckpt_save_data, out_path, epoch, model_name=f"model_{epoch + 1:06d}.checkpoint",
                       model_name_torchscript=f"model_{epoch + 1:06d}.pt")
        LOGGER.info(f"epoch {epoch + 1}: acc_val={val_metrics.acc:.4f} acc_train={trn_metrics.acc:.4f} loss_val={val_metrics.loss:.6f} "
                    f"loss_train={trn_metrics.loss:.6f} lr={lr:.3g}")
        if train_opts.early_stopping and early_stop_epochs >= train_opts.early_stopping:
            LOGGER.info(f"No validation accuracy improvement after {train_opts.early_stopping} epochs. Training stopped early.")
            break
    LOGGER.info("Saving final model checkpoint")
    save_model(trainer, ckpt_save_data, out_path, epoch, model_name=constants.FINAL_MODEL_FILENAME,
               model_name_torchscript=constants.FINAL_TORCHSCRIPT_MODEL_FILENAME)
    batch_fp.close()
    val_raw.close()
    return trainer
