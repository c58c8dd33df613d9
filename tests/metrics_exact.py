"""Shared by tests/test_host_metrics.py and tests/test_gpu_metrics.py: the exactly rounded per-base mean and variance of the
golden fixture's reads (tests/golden/base_metrics.npz), computed once per process, and the error bounds both files assert.

With u = 2^-53 and n the samples a base sums (after the trims):
    mean_bound = 2 n u sum|x| / n          n u sum|x| bounds a float64 sum of n terms in any order; x2 for the division
    var_bound  = 2 n u sum(x^2) / n + 8 u (E[x^2] + mean^2)
                                           the same scheme on the squares, plus an absolute allowance for the roundings of the
                                           squares, the two divisions, the subtraction, the root and its squaring back
A value computed by direct summation must lie within the bound of the exact value, and within |ref - exact| + bound of the
reference's value `ref`, which carries the rounding of a whole-read cumulative sum instead."""
import math
from fractions import Fraction

import numpy as np

N_READS = 8
U = 2.0**-53
_SHIFT = 1100  # every float64 sample is an integer multiple of 2^-(_SHIFT + 53)
_ONE = 1 << (_SHIFT + 53)


def _as_int(v):
    m, e = math.frexp(v)
    return int(m * 9007199254740992.0) << (e + _SHIFT)


def exact_stats(x):
    """(mean, variance, sum|x|, sum x^2) of the float64 samples x: the first two exact before one rounding to float64."""
    n = len(x)
    ints = [_as_int(v) for v in x]
    s, ss = sum(ints), sum(i * i for i in ints)
    mean = Fraction(s, n * _ONE)
    return float(mean), float(Fraction(ss, n * _ONE * _ONE) - mean * mean), math.fsum(abs(v) for v in x), float(Fraction(ss, _ONE * _ONE))


def mean_bound(n, sabs):
    return 2 * n * U * sabs / n


def var_bound(n, ssq, mean):
    return 2 * n * U * ssq / n + 8 * U * (ssq / n + mean * mean)


def read_signal(fx, i):
    """Read i's normalised signal as RemoraRead.sig computes it, float64."""
    return (fx[f"r{i}_dacs"] - float(fx["shift"][i])) / float(fx["scale"][i])


_CACHE = {}


def cases(fx):
    """Every (read, trim, quantity pair) of the fixture with its reference values and the exact statistics of every base that has
    samples: a list of dicts {read, trim, mean_name, sd_name, ref_mean, ref_sd, bases: [(base, n, mean, var, sum|x|, sum x^2)]}.
    The untrimmed pair (mean, sd) is listed once, under trim index 0.  Computed once and shared; nobody changes it."""
    if "cases" in _CACHE:
        return _CACHE["cases"]
    out = []
    for t, (st, en) in enumerate(fx["trims"].tolist()):
        for i in range(N_READS):
            m = fx[f"r{i}_map"]
            sig = read_signal(fx, i).tolist()
            pairs = [("trimmean", "trimsd", fx[f"r{i}_t{t}_trimmean"], fx[f"r{i}_t{t}_trimsd"], st, en)]
            if t == 0:
                pairs.append(("mean", "sd", fx[f"r{i}_mean"], fx[f"r{i}_sd"], 0, 0))
            for mname, sname, ref_m, ref_s, a, b in pairs:
                bases = []
                for base in np.nonzero(~np.isnan(ref_m))[0].tolist():
                    x = sig[int(m[base]) + a : int(m[base + 1]) - b]
                    bases.append((base, len(x)) + exact_stats(x))
                out.append({"read": i, "trim": t, "st": a, "en": b, "mean_name": mname, "sd_name": sname, "ref_mean": ref_m, "ref_sd": ref_s,
                            "bases": bases})
    _CACHE["cases"] = out
    return out
