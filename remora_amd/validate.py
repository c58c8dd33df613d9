"""`remora validate from_remora_dataset` on the MI355X path: the chunks of a (mixed) RemoraDataset through the
fused extraction-free inference kernels and the reference's validation summary on top (accuracy, confusion
matrix, cross-entropy loss, confidence-filtered accuracy).  Mirrors src/remora/validate.py:17-293 for the
dataset flavour: VAL_METRICS, mat_to_str, compute_metrics (:42-66), add_unmodeled_labels (:69-99),
ValidationLogger (:168-293).  The host part is numpy on N x num_labels arrays; the model forward is
HipModel.infer_chunks on the stored rows (no one-hot tensor is materialised).
`remora validate from_modbams` (src/remora/validate.py:296-594) is in the second half of the file: parse_mod_bam,
process_mods_probs, validate_modbams."""
import json
import logging
from collections import namedtuple

import numpy as np

from . import RemoraError, constants
from .engine import HipModel, _torch
from .util import softmax_axis1

VAL_METRICS = namedtuple("VAL_METRICS", ("loss", "acc", "num_calls", "conf_mat", "filt_frac", "filt_acc", "filt_conf_mat",
                                         "filt_thresh"))


def mat_to_str(mat):
    return json.dumps(np.asarray(mat).tolist(), separators=(",", ":"))


def confusion_matrix(labels, preds):
    """Counts[true, predicted] over the sorted union of the classes that occur in either vector - what
    sklearn.metrics.confusion_matrix(labels, preds) returns with default arguments (validate.py:44)."""
    labels, preds = np.asarray(labels), np.asarray(preds)
    if labels.size and min(labels.min(), preds.min()) >= 0 and max(labels.max(), preds.max()) < 4096:
        k = int(max(labels.max(), preds.max())) + 1  # small non-negative class ids: one bincount, then keep what occurs
        full = np.bincount(labels.astype(np.int64) * k + preds, minlength=k * k).reshape(k, k)
        present = (full.sum(0) + full.sum(1)) > 0
        return full[present][:, present].astype(np.int64)
    classes = np.unique(np.concatenate([labels, preds]))
    n = classes.size
    idx = np.searchsorted(classes, labels) * n + np.searchsorted(classes, preds)
    return np.bincount(idx, minlength=n * n).reshape(n, n).astype(np.int64)


def compute_metrics(probs, labels, filt_frac):
    """(acc, conf_mat, filt_frac, filt_acc, filt_conf_mat, filt_thr): overall accuracy and the accuracy over the
    calls whose winning probability lies above the `filt_frac` quantile (validate.py:42-66)."""
    preds = np.argmax(probs, axis=1)
    conf = confusion_matrix(labels, preds)
    acc = (preds == labels).sum() / labels.size
    win = np.take_along_axis(probs, preds[:, None], -1)[:, 0]
    return (acc, conf) + filtered_metrics(win, preds, labels, filt_frac)


def filtered_metrics(win, preds, labels, filt_frac):
    """(filt_frac, filt_acc, filt_conf_mat, filt_thr) of the calls whose winning probability lies above the `filt_frac`
    quantile of all winning probabilities (validate.py:47-66)."""
    thr = np.quantile(win, filt_frac)
    if thr == win.max():  # everything would be filtered: nudge the threshold below the maximum
        thr *= 0.999999
    sure = win > thr
    n_sure = int(sure.sum())
    if n_sure == 0:  # all probabilities NaN
        return 1.0, np.nan, np.array([]), np.nan
    return (1 - n_sure / labels.size, int(((preds == labels) & sure).sum()) / n_sure,
            confusion_matrix(labels[sure], preds[sure]), thr)


def add_unmodeled_labels(output, unmodeled_labels):
    """Widen model outputs by the label columns the dataset has but the model does not; those columns get -1000
    so that they vanish under softmax (validate.py:69-99)."""
    unmodeled_labels = np.asarray(unmodeled_labels)
    if unmodeled_labels.size == 0:
        return output
    nobs, nlab = output.shape
    width = nlab + unmodeled_labels.size
    wide = np.full((nobs, width), -1000, dtype=output.dtype)
    wide[:, 0] = output[:, 0]
    skipped = 0
    for col in range(1, width):
        if col in unmodeled_labels:
            skipped += 1
        else:
            wide[:, col] = output[:, col - skipped]
    return wide


_RAW = ("signal", "sequence", "sequence_to_signal_mapping", "sequence_lengths", "labels")


class ValidationLogger:
    """Tab-separated validation summary lines, same columns as the reference (validate.py:168-293)."""

    HEADER = "\t".join(("Val_Type", "Epoch", "Iteration", "Accuracy", "Confusion_Matrix", "Loss", "Num_Calls",
                        "Filtered_Fraction", "Filtered_Accuracy", "Filtered_Confusion_Matrix", "Filtered_Threshold"))
    FULL_HEADER = "\t".join(["label", "class_pred", "class_probs"])

    def __init__(self, fp, full_results_fh=None):
        self.fp = fp
        self.fp.write(self.HEADER + "\n")
        self.full_fh = full_results_fh
        if self.full_fh is not None:
            self.full_fh.write(self.FULL_HEADER + "\n")

    def write_full_results(self, output, labels):
        probs = softmax_axis1(output)
        for lab, pred, row in zip(labels.tolist(), output.argmax(axis=1), probs):
            self.full_fh.write(f"{lab}\t{pred}\t{','.join(map(str, row))}\n")

    def run_validation(self, model, model_mod_bases, criterion, dataset, filt_frac=constants.DEFAULT_FILT_FRAC,
                       full_results_fh=None, disable_pbar=False, world=1):
        """All batches of `dataset` (a finite RemoraDataset) through the model -> VAL_METRICS.  `criterion` is
        a torch loss on (float32 logits, int64 labels), or None for cross entropy; the loss is the mean of the
        per-batch means, as in the reference.

        `world` > 1 (one process per GPU, torch.distributed up, `dataset` = this rank's `RemoraDataset.shard`): the
        confusion matrix is tallied per rank over the full label set and summed by the ONE collective of the path
        (dist.allreduce_counts -> RCCL all-reduce of int64[k*k]); accuracy and num_calls follow from it.  The
        confidence-filtered columns need the global quantile of the winning probabilities, so the per-chunk (label,
        call, winning probability) triples are gathered as well (12 B per chunk, bookkeeping), and the loss is the
        mean over all ranks' batches.  Every rank returns the global metrics."""
        torch = _torch()
        if criterion is None:
            criterion = torch.nn.CrossEntropyLoss()
        md = dataset.metadata
        unmodeled = np.array([i + 1 for i, mb in enumerate(md.mod_bases) if mb not in model_mod_bases])
        fused = isinstance(model, HipModel)
        if fused and self.full_fh is None and type(criterion) is torch.nn.CrossEntropyLoss and criterion.weight is None \
                and criterion.reduction == "mean" and criterion.label_smoothing == 0.0 and criterion.ignore_index == -100 \
                and md.num_labels <= 16:
            return self._run_validation_device(model, unmodeled, dataset, filt_frac, world)
        names = _RAW if fused else ("enc_kmers", "signal", "labels")
        dataset._ds_iters = None
        all_out, all_lab, losses = [], [], []
        for batch in dataset.iter_numpy_batches(return_arrays=names, copy=not fused):
            b = dict(zip(names, batch))
            labels = np.asarray(b["labels"])
            if labels.size == 0:  # trailing empty batch of a short last super batch (the reference's loss turns NaN on it)
                continue
            if fused:  # stored rows straight into the fused kernels (uploaded from the memmaps when untouched)
                out = model.infer_chunks(b["signal"], b["sequence"], b["sequence_to_signal_mapping"], b["sequence_lengths"],
                                         md.kmer_context_bases)
                out = out.cpu().numpy() if hasattr(out, "cpu") else np.asarray(out)
            else:
                device = next(model.parameters()).device
                with torch.no_grad():
                    out = model(torch.from_numpy(b["signal"]).to(device), torch.from_numpy(b["enc_kmers"]).to(device))
                out = out.detach().cpu().numpy()
            out = add_unmodeled_labels(out, unmodeled)
            all_out.append(out)
            all_lab.append(labels)
            losses.append(criterion(torch.from_numpy(out), torch.from_numpy(np.array(labels))).detach().cpu().numpy())
            if self.full_fh is not None:
                self.write_full_results(out, labels)
        dataset._ds_iters = None
        out, labels = np.concatenate(all_out, axis=0), np.concatenate(all_lab)
        if world > 1:
            return self._global_metrics(softmax_axis1(out), labels, losses, filt_frac)
        acc, conf, ff, facc, fconf, thr = compute_metrics(softmax_axis1(out), labels, filt_frac)
        return VAL_METRICS(loss=np.mean(losses), acc=acc, num_calls=labels.size, conf_mat=conf, filt_frac=ff,
                           filt_acc=facc, filt_conf_mat=fconf, filt_thresh=thr)

    def _run_validation_device(self, model, unmodeled, dataset, filt_frac, world):
        """run_validation with the per-chunk work on the GPU (the fused model, the default loss, no per-chunk results file).
        A reader thread copies the batches' rows from the memmaps into a ring of pinned host slots (several copy threads: the
        page faults of a freshly mapped file are the slowest part of the host side) while the GPU works on the previous
        batch; the rows are uploaded on the engine's stream, inferred (fused kernels, logits stay on the device) and tallied
        there (rmr_validation_tally: widening by the unmodelled labels, float32 softmax, call, confusion counts, cross
        entropy); per chunk only the winning probability (4 B) and the call (1 B) come back, for the quantile of the
        confidence-filtered columns.  Same numbers as the host path (tests/test_gpu_parity.py)."""
        import ctypes
        import queue
        import threading
        from concurrent.futures import ThreadPoolExecutor

        from . import _lib as L
        from .util import effective_cpu_count

        torch = _torch()
        md = dataset.metadata
        eng, dev = model.engine, model.engine.torch_device
        kf, km = md.num_labels, model.num_out
        col, label_of_column = 0, []
        for c in range(kf):
            if c in set(np.asarray(unmodeled).tolist()):
                label_of_column.append(-1)
            else:
                label_of_column.append(col)
                col += 1
        if col != km:
            from . import RemoraError

            raise RemoraError(f"model has {km} outputs, the dataset's labels minus the unmodelled ones {col}")
        colmap = (ctypes.c_int32 * kf)(*label_of_column)
        conf = torch.zeros(kf * kf, dtype=torch.int64, device=dev)
        loss_buf = torch.zeros(4096, dtype=torch.float64, device=dev)
        lib = L.lib()

        import os

        depth = 3
        nthreads = max(2, min(8, effective_cpu_count() // 2))
        free, ready = queue.Queue(), queue.Queue(maxsize=depth)
        slots = [None] * depth
        for i in range(depth):
            free.put(i)
        pool = ThreadPoolExecutor(max_workers=nthreads)
        dataset._ds_iters = None

        stop = threading.Event()  # set by the consumer when it leaves early: the reader must not stay parked on a queue

        def take_free():
            while not stop.is_set():
                try:
                    return free.get(timeout=0.1)
                except queue.Empty:
                    continue
            return None

        def hand_over(item):
            while not stop.is_set():
                try:
                    return ready.put(item, timeout=0.1)
                except queue.Full:
                    continue

        def produce():
            try:
                for batch in dataset.iter_numpy_batches(return_arrays=_RAW, copy=False):
                    n = int(np.asarray(batch[4]).shape[0])
                    if n == 0:
                        continue
                    i = take_free()
                    if i is None:
                        return
                    if slots[i] is None or any(t.shape[0] < n or t.shape[1:] != np.asarray(a).shape[1:] for t, a in zip(slots[i], batch)):
                        slots[i] = [torch.empty(np.asarray(a).shape, dtype=torch.from_numpy(np.empty(0, np.asarray(a).dtype)).dtype,
                                                pin_memory=True) for a in batch]
                    parts = [(lo, min(lo + (n + nthreads - 1) // nthreads, n)) for lo in range(0, n, (n + nthreads - 1) // nthreads)]
                    views = [t.numpy() for t in slots[i]]
                    list(pool.map(lambda p: [np.copyto(v[p[0] : p[1]], a[p[0] : p[1]]) for v, a in zip(views, batch)], parts))
                    hand_over((i, n))
                hand_over(None)
            except BaseException as e:  # noqa: BLE001 - handed to the consumer
                hand_over(e)

        th = threading.Thread(target=produce, daemon=True)
        th.start()
        # the kernels run on the ENGINE's stream: that is the stream the uploads have to be ordered in front of (the caller's
        # current torch stream is the same one unless somebody changed it after the engine was made)
        main_stream = (torch.cuda.ExternalStream(eng.stream_ptr, device=dev) if getattr(eng, "stream_ptr", None)
                       else torch.cuda.current_stream(dev))
        up_stream = torch.cuda.Stream(dev)
        wins, preds, labs, sizes = [], [], [], []
        try:
            while True:
                item = ready.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                i, n = item
                # upload on a stream of its own: batch b + 1 crosses PCIe under the kernels of batch b
                with torch.cuda.stream(up_stream):
                    sig, seq, smap, lens, lab = (t[:n].to(dev, non_blocking=True) for t in slots[i])
                    up = torch.cuda.Event()
                    up.record(up_stream)
                main_stream.wait_event(up)
                for t in (sig, seq, smap, lens, lab):
                    t.record_stream(main_stream)
                labs.append(slots[i][4][:n].numpy().copy())
                logits = model.infer_chunks(sig, seq, smap, lens, md.kmer_context_bases)
                win = torch.empty(n, dtype=torch.float32, device=dev)
                pred = torch.empty(n, dtype=torch.uint8, device=dev)
                b = len(sizes)
                if b >= loss_buf.numel():
                    loss_buf = torch.cat([loss_buf, torch.zeros_like(loss_buf)])
                L.check(lib.rmr_validation_tally(eng.handle, logits.data_ptr(), lab.data_ptr(), n, km, kf, colmap, conf.data_ptr(),
                                                 win.data_ptr(), pred.data_ptr(), loss_buf.data_ptr() + 8 * b))
                wins.append(win)
                preds.append(pred)
                sizes.append(n)
                up.synchronize()  # the uploads of this slot are done: the reader may refill it under the kernels
                free.put(i)
        finally:
            stop.set()  # a consumer that raised leaves no reader behind holding pinned slots and open memmaps
            th.join(timeout=30.0)
            dataset._ds_iters = None
            pool.shutdown(wait=True)
        torch.cuda.synchronize(dev)
        win = torch.cat(wins).cpu().numpy()
        pred = torch.cat(preds).cpu().numpy().astype(np.int64)
        labels = np.concatenate(labs)
        losses = list((loss_buf[: len(sizes)].cpu().numpy() / np.asarray(sizes, np.float64)))
        full = conf.cpu().numpy().reshape(kf, kf)
        if world > 1:
            return self._global_metrics_from(kf, pred, win, labels, losses, filt_frac, local_conf=full.reshape(-1))
        present = (full.sum(0) + full.sum(1)) > 0
        ff, facc, fconf, thr = filtered_metrics(win, pred, labels, filt_frac)
        return VAL_METRICS(loss=np.mean(losses), acc=np.trace(full) / labels.size, num_calls=labels.size,
                           conf_mat=full[present][:, present], filt_frac=ff, filt_acc=facc, filt_conf_mat=fconf, filt_thresh=thr)

    @staticmethod
    def _global_metrics(probs, labels, losses, filt_frac):
        """This rank's calls -> the metrics of all ranks' calls (see run_validation)."""
        preds = np.argmax(probs, axis=1)
        win = np.take_along_axis(probs, preds[:, None], -1)[:, 0]
        return ValidationLogger._global_metrics_from(probs.shape[1], preds, win, labels, losses, filt_frac)

    @staticmethod
    def _global_metrics_from(k, preds, win, labels, losses, filt_frac, local_conf=None):
        from . import dist as rdist

        local = local_conf if local_conf is not None else np.bincount(labels.astype(np.int64) * k + preds, minlength=k * k)
        full = np.asarray(rdist.allreduce_counts(np.asarray(local, np.int64))).reshape(k, k)  # the collective: confusion counts over all GPUs
        present = (full.sum(0) + full.sum(1)) > 0
        conf = full[present][:, present]
        total = int(full.sum())
        acc = np.trace(full) / total
        lp = rdist.gather_arrays(np.stack([labels.astype(np.int64), preds.astype(np.int64)], axis=1))
        g_lab, g_pred, g_win = lp[:, 0], lp[:, 1], rdist.gather_arrays(win)  # win keeps its dtype: same quantile as one process
        loss = float(np.mean(rdist.gather_arrays(np.asarray(losses, np.float64).reshape(-1))))
        thr = np.quantile(g_win, filt_frac)
        if thr == g_win.max():
            thr *= 0.999999
        sure = g_win > thr
        n_sure = int(sure.sum())
        if n_sure == 0:
            return VAL_METRICS(loss=loss, acc=acc, num_calls=total, conf_mat=conf, filt_frac=1.0, filt_acc=np.nan,
                               filt_conf_mat=np.array([]), filt_thresh=np.nan)
        return VAL_METRICS(loss=loss, acc=acc, num_calls=total, conf_mat=conf, filt_frac=1 - n_sure / total,
                           filt_acc=(g_pred[sure] == g_lab[sure]).sum() / n_sure,
                           filt_conf_mat=confusion_matrix(g_lab[sure], g_pred[sure]), filt_thresh=thr)

    def validate_model(self, model, model_mod_bases, criterion, dataset, filt_frac=constants.DEFAULT_FILT_FRAC,
                       val_type="val", nepoch=0, niter=0, disable_pbar=False, world=1):
        ms = self.run_validation(model, model_mod_bases, criterion, dataset, filt_frac, disable_pbar=disable_pbar, world=world)
        self.fp.write(f"{val_type}\t{nepoch}\t{niter}\t{ms.acc:.6f}\t{mat_to_str(ms.conf_mat)}\t{ms.loss:.6f}\t"
                      f"{ms.num_calls}\t{ms.filt_frac:.4f}\t{ms.filt_acc:.6f}\t{mat_to_str(ms.filt_conf_mat)}\t"
                      f"{ms.filt_thresh}\n")
        return ms


# ---- `validate from_modbams` (src/remora/validate.py:296-594): modified-base calls read back from BAM files and scored at
# ground-truth sites.  The reference loops over get_aligned_pairs(with_seq=True) per base of every read in Python; here a
# batch of records is tokenised on native threads (rmr_mod_tags_sizes / _fill) and joined with the alignment and the truth
# table on the GPU (rmr_modbam_site_counts / _fill, csrc/k_modbam.hip). ----
LOGGER = logging.getLogger("Remora")

MODBAM_STATUS = {1: "no MM tag", 2: "malformed modified-base tags", 3: "unmapped", 4: "no MD tag", 5: "no modified base of the alphabet"}
FULL_RESULTS_REFUSAL = ("--full-results-filename (the per-pair alignment-context table) is not built for `validate from_modbams`: "
                        "run without it")


def _upload(torch, dev, arrays):
    """Host arrays -> ONE device buffer (a single copy across PCIe); returns the buffer and each array's device address."""
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.nbytes + 15) // 16 * 16
    host = np.empty(max(total, 16), np.uint8)
    for a, o in zip(arrays, offs):
        if a.nbytes:
            host[o : o + a.nbytes] = a.reshape(-1).view(np.uint8)
    buf = torch.from_numpy(host).to(dev)
    return buf, [buf.data_ptr() + o for o in offs]


class ModBamTruth:
    """The ground-truth sites of one BAM's reference dictionary, resident on the device: per (ref_id, strand) an ascending
    int64 position array with the label (index into `alphabet`) of every site."""

    def __init__(self, ref_names, gt_sites, alphabet, device):
        torch = _torch()
        index = {m: i for i, m in enumerate(alphabet)}
        off, pos, lab = [0], [], []
        for name in ref_names:
            for strand in "+-":
                sites = gt_sites.get((name, strand)) if hasattr(gt_sites, "get") else None
                if sites:
                    p = np.fromiter(sites.keys(), np.int64, len(sites))
                    try:
                        v = np.fromiter((index[m] for m in sites.values()), np.uint8, len(sites))
                    except KeyError as e:
                        raise RemoraError(f"Ground truth label {e} is not in the alphabet {alphabet}")
                    order = np.argsort(p, kind="stable")
                    pos.append(p[order])
                    lab.append(v[order])
                off.append(off[-1] + (len(sites) if sites else 0))
        self.n_refs = len(ref_names)
        self.off = torch.from_numpy(np.asarray(off, np.int64)).to(device)
        self.pos = torch.from_numpy(np.concatenate(pos) if pos else np.zeros(1, np.int64)).to(device)
        self.lab = torch.from_numpy(np.concatenate(lab) if lab else np.zeros(1, np.uint8)).to(device)


def tokenise_mod_tags(raw, raw_off, tags_off, threads=None):
    """rmr_mod_tags_sizes + rmr_mod_tags_fill for the records of a batch: (status i32[n], ent_off, delta_off, ml_off i64[n+1],
    entries (numpy records, _lib.MOD_ENTRY_FIELDS), deltas i32, ml u8)."""
    import ctypes

    from . import _lib as L
    from .util import effective_cpu_count

    lib = L.lib()
    # a batch of 512 records is half a millisecond of parsing: beyond four threads their start costs more than they save
    threads = max(1, min(4, effective_cpu_count())) if threads is None else int(threads)
    raw_off, tags_off = np.ascontiguousarray(raw_off, np.int64), np.ascontiguousarray(tags_off, np.int64)
    n = int(tags_off.size)
    raw_arr = np.frombuffer(raw, np.uint8) if len(raw) else np.zeros(1, np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    status = np.zeros(n, np.int32)
    sizes = np.zeros((3, max(n, 1)), np.int64)
    L.check(lib.rmr_mod_tags_sizes(n, p(raw_arr), p(raw_off), p(tags_off), p(status), p(sizes[0]), p(sizes[1]), p(sizes[2]), threads))
    offs = np.zeros((3, n + 1), np.int64)
    np.cumsum(sizes[:, :n], axis=1, out=offs[:, 1:])
    entries = np.zeros(max(int(offs[0, n]), 1), np.dtype(L.MOD_ENTRY_FIELDS))
    deltas = np.zeros(max(int(offs[1, n]), 1), np.int32)
    ml = np.zeros(max(int(offs[2, n]), 1), np.uint8)
    L.check(lib.rmr_mod_tags_fill(n, p(raw_arr), p(raw_off), p(tags_off), p(status), p(offs[0]), p(offs[1]), p(offs[2]), p(entries),
                                  p(deltas), p(ml), threads))
    return status, offs[0], offs[1], offs[2], entries[: int(offs[0, n])], deltas[: int(offs[1, n])], ml[: int(offs[2, n])]


def modbam_device_batch(dev, mod_codes, seq, seq_off, cigar, cigar_off, flag, ref_id, pos, has, tok):
    """The records of a batch and their tokenised tags on the device as an rmr_modbam_batch without its truth fields:
    (the buffer that owns the arrays, the struct)."""
    from . import _lib as L

    torch = _torch()
    status, ent_off, _, _, entries, deltas, ml = tok
    n = int(np.asarray(flag).size)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)  # noqa: E731
    i64 = lambda a: np.ascontiguousarray(a, np.int64)  # noqa: E731
    seq_arr = np.frombuffer(seq, np.uint8) if not isinstance(seq, np.ndarray) else seq
    arrays = [seq_arr, i64(seq_off), np.ascontiguousarray(cigar, np.uint32), i64(cigar_off), i32(flag), i32(ref_id), i32(pos),
              np.ascontiguousarray(has, np.uint8), i32(status), i64(ent_off), entries.view(np.uint8), i32(deltas),
              np.ascontiguousarray(ml, np.uint8)]
    buf, ptrs = _upload(torch, dev, arrays)
    b = L.ModbamBatch()
    b.n_records = n
    for name, ptr in zip(("seq", "seq_off", "cigar", "cigar_off", "flag", "ref_id", "pos", "has", "tok_status", "ent_off", "entries",
                          "deltas", "ml"), ptrs):
        setattr(b, name, ptr)
    b.n_deltas, b.n_ml, b.n_mods, b.mod_codes = int(deltas.size), int(ml.size), len(mod_codes), "".join(mod_codes).encode()
    return buf, b


def modbam_batch_sites(eng, truth, mod_codes, seq, seq_off, cigar, cigar_off, flag, ref_id, pos, has, tok):
    """The site join of one batch (rmr_modbam_site_counts, prefix sum, rmr_modbam_site_fill): device tensors probs f32[n, 1 +
    len(mod_codes)], label u8[n], qpos, rpos i64[n], and on the host the calls per record (i64) and the records' status."""
    import ctypes

    from . import _lib as L

    torch, lib, dev = _torch(), L.lib(), eng.torch_device
    deltas = tok[5]
    n, n_alpha = int(np.asarray(flag).size), len(mod_codes) + 1
    buf, b = modbam_device_batch(dev, mod_codes, seq, seq_off, cigar, cigar_off, flag, ref_id, pos, has, tok)
    b.n_refs, b.truth_off, b.truth_pos, b.truth_label = truth.n_refs, truth.off.data_ptr(), truth.pos.data_ptr(), truth.lab.data_ptr()
    n_cig = int(np.asarray(cigar).size)
    ords = torch.empty(max(int(deltas.size), 1), dtype=torch.int32, device=dev)
    cig_qr = torch.empty((2, max(n_cig, 1)), dtype=torch.int64, device=dev)
    counts = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    d_status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    L.check(lib.rmr_modbam_site_counts(eng.handle, ctypes.byref(b), ords.data_ptr(), cig_qr[0].data_ptr(), cig_qr[1].data_ptr(),
                                       counts.data_ptr(), d_status.data_ptr()))
    eng.synchronize()
    h_counts, h_status = counts[:n].cpu().numpy(), d_status[:n].cpu().numpy()
    out_off = np.zeros(n + 1, np.int64)
    np.cumsum(h_counts, out=out_off[1:])
    total = int(out_off[n])
    probs = torch.empty((max(total, 1), n_alpha), dtype=torch.float32, device=dev)
    label = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
    qr = torch.empty((2, max(total, 1)), dtype=torch.int64, device=dev)
    if total:
        d_off = torch.from_numpy(out_off).to(dev)
        L.check(lib.rmr_modbam_site_fill(eng.handle, ctypes.byref(b), ords.data_ptr(), cig_qr[0].data_ptr(), cig_qr[1].data_ptr(),
                                         d_status.data_ptr(), d_off.data_ptr(), probs.data_ptr(), label.data_ptr(), qr[0].data_ptr(),
                                         qr[1].data_ptr()))
        eng.synchronize()  # the inputs (buf, the workspaces) may go once the kernels are through
    return probs[:total], label[:total], qr[0, :total], qr[1, :total], h_counts, h_status


MOD_NOT_IN_TRUTH = ("Modified base found in BAM ({}) not found in ground truth. If this should be included in validation, add with "
                    "--extra-bases.")


def warn_ignored_entries(entries, alphabet, warn, mod_message=MOD_NOT_IN_TRUTH):
    """The one warning each for the entries of a batch that do not count: '-'-strand (duplex) entries, and a code outside the
    alphabet.  `warn`: {"strand": bool, "mod": bool}, what has not been said yet."""
    if warn["strand"] and entries.size and (entries["strand"] == b"-").any():
        LOGGER.warning("Reverse strand (duplex) mods not supported ")
        warn["strand"] = False
    if warn["mod"] and entries.size:
        fwd = entries[entries["strand"] == b"+"]
        seen = set(np.unique(np.frombuffer(fwd["codes"].tobytes(), np.uint8)).tobytes().decode("latin-1")) - {"\x00"}
        seen |= {str(c) for c in np.unique(fwd["chebi"]).tolist() if c}
        for mod_name in sorted(seen - set(alphabet)):
            LOGGER.warning(mod_message.format(mod_name))
            warn["mod"] = False
            break


def parse_mod_bam(bam_path, gt_sites, gt_ranges, alphabet, full_fh, context_bases=5, max_sites=None, device=None, batch=512,
                  return_sites=False):
    """Probabilities and ground-truth labels of every modified-base call of `bam_path` that falls on a ground-truth site
    (src/remora/validate.py:449-510): (probs float64[n, len(alphabet)], labels int64[n]), reads in file order, a read's calls
    in the order of its aligned pairs.  `alphabet`: the canonical base followed by the modified bases' single-letter codes;
    other modified bases in the BAM are ignored.  `max_sites`: at most that many calls per read, drawn with
    np.random.choice(len, size=max_sites, replace=False) read by read as the reference does.  `full_fh` must be None (the
    per-pair table is not built); `gt_ranges` and `context_bases` only serve that table.  `return_sites`: also the stored query
    position and the reference position of every call and the calls per record (before `max_sites`)."""
    from .engine import get_engine
    from .io import _readahead, bam_reference_names, iter_bam_raw_batches

    if full_fh is not None:
        raise RemoraError(FULL_RESULTS_REFUSAL)
    mods = list(alphabet[1:])
    if not 1 <= len(mods) <= 7 or any(len(m) != 1 for m in alphabet):
        raise RemoraError(f"validate from_modbams takes 1 to 7 single-letter modified bases beside the canonical base, got {alphabet}")
    torch = _torch()
    eng = get_engine(device)
    truth = ModBamTruth(bam_reference_names(bam_path), gt_sites, list(alphabet), eng.torch_device)
    parts, counts, skipped, n_records = [], [], {}, 0
    warn = {"strand": True, "mod": True}

    def tokenised():  # the reader and the tokeniser of batch k + 1 run on a thread of their own beside the join of batch k
        for rb, _ in iter_bam_raw_batches(bam_path, want_ref=False, batch=int(batch)):
            yield rb, tokenise_mod_tags(rb.raw, rb.raw_off, rb.tags_off)

    for rb, tok in _readahead(tokenised(), depth=2):
        warn_ignored_entries(tok[4], alphabet, warn)
        out = modbam_batch_sites(eng, truth, mods, rb.seq, rb.seq_off, rb.cigar, rb.cigar_off, rb.flag, rb.ref_id, rb.pos, rb.has, tok)
        parts.append(out[:4])
        counts.append(out[4])
        n_records += rb.n
        for st, k in zip(*np.unique(out[5], return_counts=True)):
            if st:
                skipped[int(st)] = skipped.get(int(st), 0) + int(k)
    for st, k in sorted(skipped.items()):
        LOGGER.info(f"{k} of {n_records} records skipped: {MODBAM_STATUS.get(st, st)} ({bam_path})")
    counts = np.concatenate(counts) if counts else np.zeros(0, np.int64)
    if int(counts.sum()) < 1:
        raise RemoraError(f"No valid modification calls from {bam_path}. Confirm that contig names from reference FASTA and ground "
                          "truth BED match.")
    probs = torch.cat([p[0] for p in parts]).cpu().numpy().astype(np.float64)
    labels = torch.cat([p[1] for p in parts]).cpu().numpy().astype(np.int64)
    keep = None
    if max_sites is not None and counts.size and int(counts.max()) > max_sites:
        start = np.concatenate([[0], np.cumsum(counts)])
        pieces = []
        for r in range(counts.size):  # read by read in file order: the reference's sequence of draws
            k = int(counts[r])
            pieces.append(start[r] + (np.random.choice(k, size=max_sites, replace=False) if k > max_sites else np.arange(k)))
        keep = np.concatenate(pieces).astype(np.int64)
    LOGGER.debug(f"Parsed {labels.size if keep is None else keep.size} modified base calls from file: {bam_path}")
    if return_sites:
        qpos = torch.cat([p[2] for p in parts]).cpu().numpy()
        rpos = torch.cat([p[3] for p in parts]).cpu().numpy()
        if keep is not None:
            return probs[keep], labels[keep], qpos[keep], rpos[keep], counts
        return probs, labels, qpos, rpos, counts
    return (probs, labels) if keep is None else (probs[keep], labels[keep])


def process_mods_probs(probs, labels, allow_unbalanced, pct_filt, name):
    """The summary line of `validate from_modbams` (src/remora/validate.py:102-154): classes balanced to the smallest one that
    occurs (np.random.shuffle of the larger ones) unless `allow_unbalanced`, then compute_metrics.  Logged as the reference
    logs it; the text is returned as well."""
    if not allow_unbalanced:
        nlabs = max(labels.max() + 1, probs.shape[1])
        labels_probs = [probs[labels == mod_idx] for mod_idx in range(nlabs)]
        lab_sizes = [lp.shape[0] for lp in labels_probs]
        if len(lab_sizes) == 1:
            raise RemoraError("Cannot balance dataset with 1 label. Consider running with `--allow-unbalanced`")
        LOGGER.debug(f"Balancing labels. Starting from: {lab_sizes}")
        min_size = min([s for s in lab_sizes if s > 0])
        bal_probs, bal_labels = [], []
        for lab_idx, label_probs in enumerate(labels_probs):
            if label_probs.shape[0] == 0:  # labels not included in ground truth
                continue
            if label_probs.shape[0] > min_size:
                np.random.shuffle(label_probs)
            bal_probs.append(label_probs[:min_size])
            bal_labels.append(np.full(min_size, lab_idx, dtype=labels.dtype))
        probs, labels = np.concatenate(bal_probs), np.concatenate(bal_labels)
    acc, conf_mat, filt_frac, filt_acc, filt_conf_mat, filt_thr = compute_metrics(probs, labels, pct_filt / 100)
    val_output = (f"\n{ValidationLogger.HEADER}\n{name}\t0\t0\t{acc:.6f}\t{mat_to_str(conf_mat)}\tNAN\t{labels.size}\t{filt_frac:.4f}\t"
                  f"{filt_acc:.6f}\t{mat_to_str(filt_conf_mat)}\t{filt_thr}\n")
    LOGGER.info(val_output)
    return val_output


def validate_modbams(bams_and_beds, full_results_path, name, pct_filt, allow_unbalanced=False, seed=None, extra_bases=None,
                     max_sites_per_read=None, device=None):
    """`validate from_modbams` (src/remora/validate.py:513-594).  The reference draws and logs `seed` without applying it; here
    np.random.seed(seed) is called once, first of all, so that the draws of --max-sites-per-read and of the balancing repeat
    under the same seed.  Returns the summary text."""
    from .io import parse_mods_bed

    seed = int(np.random.randint(0, np.iinfo(np.uint32).max, dtype=np.uint32)) if seed is None else seed
    LOGGER.debug(f"Seed selected is {seed}")
    np.random.seed(seed)
    if full_results_path is not None:
        raise RemoraError(FULL_RESULTS_REFUSAL)
    LOGGER.info("Parsing ground truth BED files")
    bams, beds = zip(*bams_and_beds)
    parsed, all_gt_sites, all_gt_ranges, all_mods = {}, [], [], set()
    for bed_path in beds:
        if bed_path not in parsed:
            parsed[bed_path] = parse_mods_bed(bed_path)
            tot_sites = sum(len(cs_sites) for cs_sites in parsed[bed_path][0].values())
            LOGGER.info(f"Parsed {tot_sites} total sites with labels {parsed[bed_path][1]} from {bed_path}")
        gt_sites, samp_mods = parsed[bed_path]
        all_gt_sites.append(gt_sites)
        all_gt_ranges.append(dict((cs, (min(poss), max(poss))) for cs, poss in gt_sites.items()))
        all_mods.update(samp_mods)
    if extra_bases is not None:
        all_mods.update(extra_bases)
    can_base = all_mods.intersection("ACGTU")
    if len(can_base) > 1:
        raise RemoraError(f"More than one canonical base found: {can_base}")
    if len(can_base) == 0:
        raise RemoraError("No canonical bases found in ground truth.")
    alphabet = list(can_base) + sorted(all_mods.difference("ACGTU"))
    LOGGER.info("Parsing modBAM files")
    all_probs, all_labels = [], []
    for bam_path, gt_sites, gt_ranges in zip(bams, all_gt_sites, all_gt_ranges):
        probs, labels = parse_mod_bam(bam_path, gt_sites, gt_ranges, alphabet, None, max_sites=max_sites_per_read, device=device)
        all_probs.append(probs)
        all_labels.append(labels)
    LOGGER.info(f"Alphabet used (and order of reported metrics): {alphabet}")
    return process_mods_probs(np.vstack(all_probs), np.concatenate(all_labels), allow_unbalanced, pct_filt, name)
