"""CPU-side pieces of `model train`: the C ABI of the trainer is declared, exported and bound; RollingMAD and the cool-down
scheduler against values worked out here; the architecture scan of a --model file; argument parsing; remora_amd.nets against
a stored trained network."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden

TRAINER_ENTRIES = ["rmr_trainer_adamw_step", "rmr_trainer_create", "rmr_trainer_destroy", "rmr_trainer_forward_backward",
                   "rmr_trainer_grad_absmax", "rmr_trainer_read", "rmr_trainer_tensor_layout", "rmr_trainer_write"]


def test_trainer_entry_points_declared_exported_and_bound():
    from remora_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "remora_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rmr_trainer_[a-z_0-9]+)\s*\(", hdr)))
    assert declared == TRAINER_ENTRIES
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in TRAINER_ENTRIES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    # the buffer selectors of the binding are the header's
    for i, name in enumerate(("PARAMS", "GRADS", "ADAM_M", "ADAM_V", "COUNTERS")):
        assert re.search(rf"RMR_TRAIN_{name} = {i}\b", hdr) and getattr(_lib, f"TRAIN_{name}") == i
    assert re.search(r"#define RMR_TRAIN_NAME_LEN (\d+)", hdr).group(1) == str(_lib.TRAIN_NAME_LEN)
    # the training kernels are registered with the engine's profiler
    names = [lib.rmr_profile_kernel_name for _ in range(1)][0]
    names.restype = ctypes.c_char_p
    lib.rmr_profile_num_kernels.restype = ctypes.c_int
    kernels = [names(i).decode() for i in range(lib.rmr_profile_num_kernels())]
    for k in ("train_gemm", "train_wgrad", "train_reduce", "train_bn", "train_lstm", "train_loss", "train_adamw", "train_aux"):
        assert k in kernels, k
    assert "?" not in kernels
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"train_gemm_kernel" in blob and b"train_wgrad_kernel" in blob


def test_rolling_mad_against_worked_values():
    from remora_amd.train_model import RollingMAD, med_mad

    r = RollingMAD(2, n_mads=2, window=4)
    assert r.nparams == 2 and r.window == 4
    assert r.update([1.0, 10.0]) is None and r.update([2.0, 10.0]) is None and r.update([4.0, 10.0]) is None
    # window full: row 0 = [1, 2, 4, 8] -> median 3, |x - 3| = [2, 1, 1, 5] -> median 1.5, MAD 1.4826 * 1.5; row 1 constant
    thr = r.update([8.0, 10.0])
    assert np.allclose(thr, [3.0 + 2 * 1.4826 * 1.5, 10.0])
    # the window rolls: the oldest value (1) is replaced by 16 -> [16, 2, 4, 8]: median 6, deviations [10, 4, 2, 2] -> median 3
    thr = r.update([16.0, 10.0])
    assert np.allclose(thr, [6.0 + 2 * 1.4826 * 3.0, 10.0])
    with pytest.raises(Exception):
        r.update([1.0])
    med, mad = med_mad(np.array([1.0, 2.0, 4.0, 8.0]))
    assert med == 3.0 and np.isclose(mad, 1.4826 * 1.5)
    assert RollingMAD(3, 0, window=1, default_to=7).update([1, 2, 3]).tolist() == [1, 2, 3]  # n_mads 0: the median itself


def test_high_conf_incorrect_mask():
    from remora_amd.train_model import high_conf_incorrect_mask

    big = np.log(np.array([[0.99, 0.01], [0.01, 0.99], [0.6, 0.4], [0.95, 0.05], [0.2, 0.8]]))
    labels = np.array([1, 1, 1, 1, 1])  # rows 0, 2, 3 are called wrong, with 0.99, 0.6 and 0.95
    # room for two rows to leave: the two confident wrong calls do, the 0.6 one stays
    assert high_conf_incorrect_mask(big, labels, 0.9, 0.4).tolist() == [False, True, True, False, True]
    # a threshold nobody reaches: every row stays
    assert high_conf_incorrect_mask(big, labels, 0.999, 0.4).all()


def test_cool_down_scheduler_against_worked_values():
    from remora_amd.model_util import TrainOpts

    opts = TrainOpts(epochs=4, lr_scheduler_str="CosineAnnealingLR", lr_scheduler_kwargs=(("T_max", 4, "int"), ("eta_min", 0.0, "float")),
                     lr_cool_down_epochs=2, lr_cool_down_lr=1e-7, opt_kwargs=(("lr", 0.5, "float"),), learning_rate=123.0)
    assert opts.optimizer_kwargs() == {"lr": 0.5}  # --lr (learning_rate) does not reach the optimiser
    sch = opts.load_scheduler(opts.load_optimizer())
    assert sch.total_epochs == 6
    seen = []
    for _ in range(6):
        seen.append(sch.lr)
        sch.step()
    # the 4 epochs run at the cosine's values (eta_min 0: lr (1 + cos(pi e / T_max)) / 2), the 2 cool-down epochs at 1e-7
    cos = [0.5 * 0.5 * (1 + np.cos(np.pi * e / 4)) for e in range(4)]
    assert np.allclose(seen[:4], cos) and seen[4:] == [1e-7, 1e-7], seen
    assert sch.get_last_lr() == [1e-7]
    # the default run: AdamW's own 1e-3 with weight decay 1e-4
    d = TrainOpts()
    assert d.optimizer_kwargs() == {"weight_decay": 1e-4} and d.load_optimizer().param_groups[0]["lr"] == 1e-3
    from remora_amd import RemoraError

    with pytest.raises(RemoraError, match="AdamW only"):
        TrainOpts(optimizer_str="SGD").optimizer_kwargs()
    with pytest.raises(RemoraError, match="momentum"):
        TrainOpts(opt_kwargs=(("momentum", 0.9, "float"),)).optimizer_kwargs()


def _model_file(path, names, style="plain"):
    with open(path, "w") as fh:
        fh.write("raise SystemExit('never executed')\nfrom torch import nn\n\n\nclass network(nn.Module):\n    def __init__(self, size=64):\n        super().__init__()\n")
        for n in names:
            fh.write(f"        self.{n} = nn.Identity()\n" if style == "plain" else f"        self.{n}, self.{n}_twin = nn.Identity(), None\n")
    return str(path)


def test_model_file_scan(tmp_path):
    from remora_amd import RemoraError
    from remora_amd.model_util import scan_model_file

    lstm = ["sig_conv1", "sig_bn1", "sig_conv2", "sig_conv3", "seq_conv1", "seq_conv2", "merge_conv1", "merge_bn", "lstm1", "lstm2", "fc", "dropout"]
    conv = ["sig_conv1", "sig_conv2", "sig_conv3", "seq_conv1", "seq_conv2", "seq_conv3", "merge_conv1", "merge_conv2", "merge_conv3", "merge_conv4", "fc"]
    assert scan_model_file(_model_file(tmp_path / "a.py", lstm)) == "conv_lstm"
    assert scan_model_file(_model_file(tmp_path / "b.py", lstm, style="tuple")) == "conv_lstm"
    assert scan_model_file(_model_file(tmp_path / "c.py", conv)) == "conv_only"
    with pytest.raises(RemoraError, match="unknown layer set"):
        scan_model_file(_model_file(tmp_path / "d.py", lstm[:-4]))
    bad = tmp_path / "e.py"
    bad.write_text("class network(:\n")
    with pytest.raises(RemoraError, match="cannot parse"):
        scan_model_file(str(bad))


def test_model_train_argument_parsing():
    from remora_amd import constants
    from remora_amd.__main__ import build_parser

    ap = build_parser()
    a = ap.parse_args(["model", "train", "DS", "--model", "m.py"])
    assert a.remora_dataset_path == "DS" and a.batch_size == constants.DEFAULT_BATCH_SIZE == 2048 and a.size == 64
    assert a.epochs == 100 and a.early_stopping == 10 and a.optimizer == "AdamW" and a.lr == 1e-3 and a.lr_scheduler == "CosineAnnealingLR"
    assert a.gradient_clip_num_mads == 0 and a.high_conf_incorrect_thr_frac is None and a.ext_val is None and a.seed is None
    assert a.chunks_per_epoch == 10_000_000 and a.num_test_chunks == 10_000 and a.save_freq == 10 and a.filter_fraction == 0.1
    assert a.output_path == "remora_train_results" and not a.overwrite and a.finetune_path is None and a.freeze_num_layers == 0
    assert a.super_batch_size == 100_000 and a.super_batch_sample_fraction == 1.0 and not a.read_batches_from_disk
    a = ap.parse_args(["model", "train", "DS", "--model", "m.py", "--gradient-clip-num-mads", "None", "--high-conf-incorrect-thr-frac", "0.9", "0.1",
                       "--ext-val", "A", "B", "--ext-val-names", "a", "b", "--optimizer-kwargs", "lr", "0.01", "float", "--chunk-context", "25", "25",
                       "--kmer-context-bases", "2", "3", "--lr-scheduler-kwargs", "T_max", "7", "int", "--device", "cuda:1"])
    assert a.gradient_clip_num_mads is None and a.high_conf_incorrect_thr_frac == [0.9, 0.1] and a.ext_val == ["A", "B"]
    assert a.optimizer_kwargs == [["lr", "0.01", "float"]] and a.chunk_context == [25, 25] and a.kmer_context_bases == [2, 3]
    assert a.lr_scheduler_kwargs == [["T_max", "7", "int"]] and a.device == "cuda:1"
    with pytest.raises(SystemExit):
        ap.parse_args(["model", "train", "DS"])  # --model is required


def test_nets_reproduces_the_trained_golden_model():
    import torch

    from remora_amd import nets

    g = golden("model_convlstm_s64_l100_o2_trained.npz")
    state = {k[3:].replace("__", "."): g[k] for k in g.files if k.startswith("w__")}
    net = nets.from_state(state)
    assert not net.training
    with torch.no_grad():
        out = net(torch.from_numpy(g["sigs"][:8]), torch.from_numpy(g["dense_seqs"])).numpy()
    assert np.abs(out - g["dense_logits"]).max() <= 1e-5
    # the same layers, names and order as the reference's network: its state loads strict, and a seed draws the same start
    a, b = nets.build(16, 5, 3, seed=9), nets.build(16, 5, 3, seed=9)
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    from oracle import torch_ref

    torch.manual_seed(9)
    ref = torch_ref.ConvLSTMRef(16, 5, 3)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), ref.state_dict().values()))
    torch.jit.script(net)  # what export_model_torchscript serialises
