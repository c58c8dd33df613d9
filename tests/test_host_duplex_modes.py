"""CPU-only tests of the aligner's memory modes (rmr_duplex_align_mode): the entry point declared, exported and bound, the mode
constants of the header and of duplex_utils held together, the footprint of an alignment in checkpointed memory, and the new
command-line option."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "remora_hip.h")).read(), flags=re.S)


def test_mode_entry_is_declared_exported_and_bound():
    from remora_amd import _lib

    decl = re.search(r"\bint rmr_duplex_align_mode\s*\(([^;]*)\)\s*;", _header())
    assert decl, "rmr_duplex_align_mode is not declared in include/remora_hip.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    restype, argtypes = _lib.SIGNATURES["rmr_duplex_align_mode"]
    assert restype is ctypes.c_int and len(argtypes) == len(args) == 14
    assert args[8] == "int mode" and argtypes[8] is ctypes.c_int  # behind the budget, in front of the outputs
    assert args[-2:] == ["int64_t *n_groups", "int64_t *n_checkpointed"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "rmr_duplex_align_mode") and hasattr(lib, "rmr_duplex_align")


def test_mode_constants_agree_with_the_header():
    from remora_amd import duplex_utils as DU

    defs = dict(re.findall(r"#define (RMR_DUPLEX_MODE_\w+) (\d+)\s", _header()))
    assert {k: int(v) for k, v in defs.items()} == {"RMR_DUPLEX_MODE_FULL": 0, "RMR_DUPLEX_MODE_CHECKPOINT": 1, "RMR_DUPLEX_MODE_AUTO": 2}
    assert (DU.MODE_FULL, DU.MODE_CHECKPOINT, DU.MODE_AUTO) == (0, 1, 2)
    assert DU.MODES == {"full": DU.MODE_FULL, "checkpoint": DU.MODE_CHECKPOINT, "auto": DU.MODE_AUTO}


def test_checkpoint_bytes():
    from remora_amd import duplex_utils as DU

    assert DU.checkpoint_bytes(513, 1000) == 2 * 1000 * 8 + 1063 * 256
    assert DU.checkpoint_bytes(1, 1) == 8 + 64 * 256 and DU.checkpoint_bytes(512, 1000) == 1000 * 8 + 1063 * 256
    # below the trace from the second strip on, whatever the duplex length (one strip: the same strip of trace plus its line)
    for n in (513, 514, 1024, 1025, 5000, 24561, 1 << 20):
        for m in (1, 2, 63, 64, 65, 1000, 24561, 1 << 20):
            assert DU.checkpoint_bytes(n, m) < DU.trace_bytes(n, m), (n, m)
    for m in (1, 1000):
        assert DU.checkpoint_bytes(512, m) == DU.trace_bytes(512, m) + 8 * m
    # the 24.5 kb fixture pair: 48 lines and a strip of trace, about a twentieth of its trace
    assert DU.checkpoint_bytes(24561, 24561) == 48 * 24561 * 8 + 24624 * 256 < DU.trace_bytes(24561, 24561) // 19


def test_unknown_mode_is_refused_before_any_call():
    import pytest

    from remora_amd import RemoraError
    from remora_amd import duplex_utils as DU

    with pytest.raises(RemoraError, match="unknown duplex alignment mode"):
        DU.align_batch([], engine=object(), mode="banded")


def test_command_line_takes_the_trace_budget():
    from remora_amd.__main__ import build_parser

    base = "infer duplex_from_pod5_and_bam a b c d --model m.pt --out-bam o.bam"
    assert build_parser().parse_args(base.split()).duplex_trace_gib == 16.0
    assert build_parser().parse_args((base + " --duplex-trace-gib 0.5").split()).duplex_trace_gib == 0.5
