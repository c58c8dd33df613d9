"""CPU-only tests of the Winograd guard (include/remora_hip.h, rmr_model_numerics): the two entry points are declared,
exported and bound, and the probe batch of remora_amd/csrc/rmr_probe.h - the chunks every fp32 model with a Winograd layer
is screened on at load - is the same bytes everywhere and a legal batch of chunk arrays."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

ENTRY_POINTS = ("rmr_model_numerics_get", "rmr_model_check_winograd")
# FNV-1a over signal, sequence rows, mapping rows and lengths (tests/c/probe_batch.cpp), k-mer length 9
DIGESTS = {(100, 9): "7251636e8256fe9a", (200, 9): "fa82f414fd694795"}


def test_guard_entry_points_are_declared_exported_and_bound():
    from remora_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "remora_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(rf"\bint {name}\s*\(", code), f"{name} not declared in include/remora_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in _lib.SIGNATURES
    # the struct of the header, field for field, in the ctypes binding
    body = re.search(r"typedef struct rmr_model_numerics \{(.*?)\} rmr_model_numerics;", code, flags=re.S).group(1)
    fields = re.findall(r"\b(int32_t|float)\s+(\w+);", body)
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.ModelNumerics._fields_)
    assert [n for _, n in fields] == ["checked", "winograd", "probe_chunks", "nonfinite", "max_abs_diff", "tol"]
    assert ctypes.sizeof(_lib.ModelNumerics) == 24
    # a NULL model is an error, not a crash
    rec = _lib.ModelNumerics()
    assert _lib.lib().rmr_model_numerics_get(None, ctypes.byref(rec)) != 0
    assert _lib.lib().rmr_model_check_winograd(None, ctypes.c_float(0.0), ctypes.byref(rec)) != 0


@pytest.fixture(scope="module")
def probe_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path_factory.mktemp("probe") / "probe_batch")
    cc = subprocess.run([gxx, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "remora_amd", "csrc"),
                         os.path.join(ROOT, "tests", "c", "probe_batch.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0 and not cc.stderr, cc.stderr
    return exe


@pytest.mark.parametrize("L,K", [(100, 9), (200, 9), (100, 23), (99, 6), (37, 9)])
def test_probe_batch_is_a_legal_fixed_batch_of_chunk_arrays(probe_exe, L, K):
    """Every mapping row monotone and ending at L, every length within [1, L / 5], every base 0..3 or the padding value, the
    shortest and the longest length present, noise of unit variance within +-5 (the checks of tests/c/probe_batch.cpp); at the
    two chunk lengths of the project's configurations the bytes are pinned by their digest."""
    run = subprocess.run([probe_exe, str(L), str(K)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.strip().endswith("0 failed checks"), run.stdout + run.stderr
    digest = re.search(r"digest ([0-9a-f]{16})", run.stdout).group(1)
    if (L, K) in DIGESTS:
        assert digest == DIGESTS[(L, K)]
    # the generator has no state outside the call
    again = subprocess.run([probe_exe, str(L), str(K)], capture_output=True, text=True, timeout=60)
    assert again.stdout == run.stdout


def test_probe_generator_uses_no_library_randomness():
    src = open(os.path.join(ROOT, "remora_amd", "csrc", "rmr_probe.h")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "<random>" not in code and not re.search(r"\brand\s*\(", code) and "<hip/" not in code
