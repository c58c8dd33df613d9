"""Shared by tests/test_host_model_export.py and tests/test_gpu_model_dir.py: the fixture tests/golden/dorado_export.npz (the
reference's export_model_dorado on two small models, tools/gen_golden.py gen_dorado_export) and the directories made from it."""
import functools
import json
import os

import numpy as np

from conftest import GOLDEN

TAGS = ("convlstm_s16", "conv_s24")
KCB = (4, 4)


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(os.path.join(GOLDEN, "dorado_export.npz"), allow_pickle=False)
    return {k: g[k] for k in g.files}


def state_of(tag):
    pre = f"{tag}__state__"
    return {k[len(pre):]: v for k, v in fixture().items() if k.startswith(pre)}


def ref_tensors(tag):
    """{file name: array} of the `.tensor` files the reference wrote."""
    pre = f"{tag}__tensor__"
    return {k[len(pre):]: v for k, v in fixture().items() if k.startswith(pre)}


def ref_config(tag):
    """The dict the reference handed to toml.dump, None values dropped (toml.dump leaves them out)."""
    doc = json.loads(str(fixture()[f"{tag}__config"]))
    return {t: {k: v for k, v in body.items() if v is not None} for t, body in doc.items()}


def ckpt_of(tag, with_refiner_object=False):
    """The checkpoint dict the reference exported: the entries a training checkpoint holds (`refine_*` keys); with
    `with_refiner_object` also `sig_map_refiner`, as the metadata of a loaded model file has it."""
    import torch

    from remora_amd.model_util import refiner_from_checkpoint

    g = fixture()
    ck = json.loads(str(g[f"{tag}__meta"]))
    ck["motifs"] = [tuple(m) for m in ck["motifs"]]
    ck["kmer_context_bases"], ck["chunk_context"] = tuple(ck["kmer_context_bases"]), tuple(ck["chunk_context"])
    ck["refine_kmer_levels"] = g.get(f"{tag}__refine_kmer_levels")
    ck["refine_sd_arr"] = g[f"{tag}__refine_sd_arr"]
    ck["state_dict"] = {k: torch.from_numpy(v.copy()) for k, v in state_of(tag).items()}
    if with_refiner_object:
        ck["sig_map_refiner"] = refiner_from_checkpoint(ck)
    return ck


def chunks_of(tag):
    g = fixture()
    return tuple(g[f"{tag}__{k}"] for k in ("sigs", "seqs", "maps", "lens"))


def write_reference_dir(tag, path):
    """A model directory from the reference's tensors and config, written by the project's `.tensor` and TOML writers."""
    from remora_amd import toml_lite
    from remora_amd.model_util import save_tensor_file

    os.makedirs(path, exist_ok=True)
    for name, arr in ref_tensors(tag).items():
        save_tensor_file(os.path.join(path, name), arr)
    toml_lite.dump(ref_config(tag), os.path.join(path, "config.toml"))
    return str(path)


def read_dir_tensors(path):
    from remora_amd.model_util import load_tensor_file

    return {f: load_tensor_file(os.path.join(path, f)) for f in sorted(os.listdir(path)) if f.endswith(".tensor")}
