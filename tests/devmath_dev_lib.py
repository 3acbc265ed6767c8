"""Builds and loads tests/devmath_dev/libdevmathdev.so (TEST INFRASTRUCTURE ONLY): one primitive of csrc/devmath.hpp per element,
evaluated ON THE DEVICE, built by hipcc with the product's own flag set (crychic_renderer_amd.build.FLAGS, taken from the module so
that the two cannot drift) -- and holds the inputs the three tiers (the oracle's definitions, the host build tests/hostsim, the
device) are compared on: exhaustive where the format is small, a lattice over every upper half-word plus the breakpoints of the
algorithms elsewhere.  The kind numbers are or_eval_array's (oracle/or_light.c)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "devmath_dev")
SRC, LIB = os.path.join(DIR, "devmath_dev.hip"), os.path.join(DIR, "libdevmathdev.so")
CSRC = os.path.join(ROOT, "crychic_renderer_amd", "csrc")
DEPS = [SRC, os.path.join(ROOT, "tests", "hostsim", "devmath_eval.hpp"), os.path.join(CSRC, "devmath.hpp"), os.path.join(CSRC, "gamma_pow.inc")]
MAX_CALL = 1 << 24          # dm_eval_array refuses more per call
FULL = os.environ.get("CRY_DEVMATH_FULL") == "1"      # soak: all 2^32 patterns of every unary kind, in chunks of 2^24


def build():
    from crychic_renderer_amd import build as product
    deps = DEPS + [product.__file__]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        tmp = LIB + ".tmp.%d" % os.getpid()
        try:
            subprocess.run([hipcc] + product.FLAGS + ["-I", os.path.join(ROOT, "include"), "-I", CSRC, "-x", "hip", SRC, "-o", tmp], check=True)
            os.replace(tmp, LIB)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
    return LIB


PROBE = os.path.join(ROOT, "tools", "exact_math_probe")


def build_probe():
    """tools/exact_math_probe, the all-2^32 sweeps of the reciprocal / length family, with the product's flag set as an executable."""
    from crychic_renderer_amd import build as product
    src = PROBE + ".hip"
    deps = [src, os.path.join(CSRC, "devmath.hpp"), os.path.join(CSRC, "gamma_pow.inc"), product.__file__]
    if not os.path.exists(PROBE) or any(os.path.getmtime(d) > os.path.getmtime(PROBE) for d in deps):
        flags = [f for f in product.FLAGS if f != "-shared"]
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + [src, "-o", PROBE], check=True)
    return PROBE


class DevMath:
    def __init__(self):
        self.lib = C.CDLL(build())
        self.lib.dm_eval_array.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        self.lib.dm_eval_array.restype = C.c_int

    def eval_raw(self, kind, a, b, out):
        return self.lib.dm_eval_array(kind, a.size, a.ctypes.data, b.ctypes.data, out.ctypes.data)

    def eval_array(self, kind, a, b=None):
        """The device's results as float32 (bits), in calls of at most 2^24 elements; raises on a HIP error code."""
        a = np.ascontiguousarray(a).reshape(-1)
        b = np.ascontiguousarray(b).reshape(-1) if b is not None else a
        out = np.zeros(a.shape, np.float32)
        for lo in range(0, a.size, MAX_CALL):
            rc = self.eval_raw(kind, a[lo:lo + MAX_CALL], b[lo:lo + MAX_CALL], out[lo:lo + MAX_CALL])
            if rc != 0:
                raise RuntimeError("dm_eval_array(kind %d) returned HIP error %d" % (kind, rc))
        return out


_LIB = None


def load():
    global _LIB
    if _LIB is None:
        _LIB = DevMath()
    return _LIB


# ---- kinds ---------------------------------------------------------------------------------------------------------
SIN, COS, LOG2, EXP2, POW, NRAND, D24, UNORM16, UNORM8, HALF, GAMMA, GAMMA2_Y = range(12)
RCP, RCP_NORMAL, DIVF, CLAMP_LEN2, SQRT_CLAMPED, LEN, INV_LEN = range(12, 19)
RCP2_X, RCP2_Y, RCP_NORMAL2_X, RCP_NORMAL2_Y, INV_LEN2_X, INV_LEN2_Y, GAMMA2_X = range(19, 26)
SATURATE, MAXNN, SIGN1, SIGNF, LERP_AB, LERP_BT, TO_UNORM8, TO_UNORM16, TEXEL_INDEX = range(26, 35)
BILINEAR0, MUL24 = 35, 51
SIZES = ((2, 16), (16, 130), (130, 16384), (16384, 2))        # (w, h) of kinds BILINEAR0 + 4 s + o, o = i0, j0, fx, fy


# ---- inputs (uint32 bit patterns) --------------------------------------------------------------------------------------
def f2u(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def u2f(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


@functools.lru_cache(None)
def lower_halves():
    """The 256 lower half-words of the lattice: five fixed ones and 251 drawn once."""
    fixed = [0x0000, 0x0001, 0x7FFF, 0x8000, 0xFFFF]
    rest = np.setdiff1d(np.arange(65536), fixed)
    drawn = np.random.default_rng(20240607).choice(rest, 251, replace=False)
    return np.concatenate([fixed, np.sort(drawn)]).astype(np.uint32)


@functools.lru_cache(None)
def lattice():
    """2^24 patterns: every upper half-word with each of lower_halves() -- every exponent, both signs, the subnormals, both
    infinities, quiet and signaling NaNs."""
    a = (np.arange(65536, dtype=np.uint32)[:, None] << 16) | lower_halves()[None, :]
    a = a.reshape(-1)
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def rotated():
    """The lattice rotated so that both half-words of a pair differ (the second operand, the other lane)."""
    a = np.roll(lattice(), 256 * 7919 + 101)
    a.setflags(write=False)
    return a


def neighbours(x, n=8):
    """The float32 values x and the n floats below and above each, as bits (across zero: the subnormals of the other sign)."""
    return neighbours_of_bits(f2u(np.asarray(x, np.float64).astype(np.float32).reshape(-1)), n)


def neighbours_of_bits(u, n=8):
    """neighbours() of patterns given as bits; NaN patterns and what lies beyond the infinities drop out."""
    u = np.asarray(u, np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, -(u & 0x7FFFFFFF), u)                   # monotone in the value; +0 and -0 share 0
    key = (key[:, None] + np.arange(-n, n + 1)[None, :]).reshape(-1)
    key = key[np.abs(key) <= 0x7F800000]
    return np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32)


@functools.lru_cache(None)
def breakpoints():
    """Where the algorithms of devmath.hpp change course, +- 8 ulp each."""
    k = np.concatenate([np.arange(4097), 2 ** np.arange(13, 23)]).astype(np.float64)
    quarter_turns = np.concatenate([k * (np.pi / 2), -k * (np.pi / 2), [8388608.0, -8388608.0]])       # det_sincos: k pi/2, the range limit
    e = np.arange(256, dtype=np.uint32) << 23
    cut = np.concatenate([e | 0x3504F3, e | 0x3504F3 | 0x80000000])        # det_log2_normal's mantissa cut 0x3F3504F3 at every exponent
    halves = np.concatenate([np.arange(-127, 128) + 0.5, [-125.0, 127.0]])                             # det_exp2: rint ties, the clamp ends
    buckets = np.concatenate([e, e | 0x7FFFFF, e | 0x80000000, e | 0x807FFFFF])                        # pow_inv_gamma: both ends of every exponent bucket
    q8 = (np.arange(256) + 0.5) / 255.0                                                                # float_to_unorm8 / 16: the rounding ties
    q16 = (np.arange(65536) + 0.5) / 65535.0
    texel = np.array([-2.0, -1.0, 0.0, 2.0 ** 31] + [float(d) for d in (2, 16, 130, 16384)])
    powers = np.array([s * 2.0 ** p for s in (1, -1) for p in (-126, 126, -100, 100)])
    vals = np.concatenate([quarter_turns, halves, q8, q16, texel, powers])
    u = np.concatenate([neighbours(vals), neighbours_of_bits(cut), neighbours_of_bits(buckets)])
    u = np.unique(u)
    u.setflags(write=False)
    return u


def is_nan(u):
    return (u & 0x7FFFFFFF) > 0x7F800000


def is_snan(u):
    return is_nan(u) & ((u & 0x00400000) == 0)


def exponent_between(u, lo, hi):
    """lo <= |x| <= hi for lo = 2^a, hi = 2^b given as exponents (a, b): on the bits, no float compare."""
    m = u & 0x7FFFFFFF
    return (m >= np.uint32((lo + 127) << 23)) & (m <= np.uint32((hi + 127) << 23))


# the stated domains: predicates on the INPUT bits, and the number of lattice points each keeps, worked out by hand
#   2^-126 <= |b| <= 2^126: exponent fields 1 .. 252 in full (128 upper half-words each, 256 lower ones) and 2^126 itself, both signs
#   [2^-100, 2^100]: exponent fields 27 .. 226 and 2^100 itself, positive
#   no signaling NaN: upper half-words 0x7F80 (lower half-word not 0: 255) and 0x7F81 .. 0x7FBF (63), both signs
DOMAINS = {
    "rcp_normal": (lambda a: exponent_between(a, -126, 126), 2 * (252 * 128 * 256 + 1), lambda x: (np.abs(x) >= 2.0 ** -126) & (np.abs(x) <= 2.0 ** 126)),
    "sqrt_clamped": (lambda a: exponent_between(a, -100, 100) & (a < 0x80000000), 200 * 128 * 256 + 1, lambda x: (x >= 2.0 ** -100) & (x <= 2.0 ** 100)),
    "no_snan": (lambda a: ~is_snan(a), (1 << 24) - 2 * (255 + 63 * 256), None),
    None: (lambda a: np.ones(a.shape, bool), 1 << 24, None),
}


class Case:
    """One comparison: kind(a, b) on the kept inputs.  `kept` is the number of inputs the domain's predicate must keep (asserted by
    the tests), `integer`: the result is an integer's bits (compared exactly; no NaN share), `cap`: the largest share of NaN results
    the oracle may give on these inputs (a NaN equals any NaN, so NaN results are blind), None where it is not a float."""
    def __init__(self, name, kind, a, b=None, kept=None, integer=False, cap=0.005):
        self.name, self.kind, self.a, self.b, self.integer, self.cap = name, kind, a, b, integer, None if integer else cap
        self.kept = a.size if kept is None else kept


def _unary(name, kind, domain=None, other_lane=False, **kw):
    """The lattice and the breakpoints through a unary kind (other_lane: the rotated copy goes into the packed form's other lane)."""
    pred, lattice_kept, real_pred = DOMAINS[domain]
    a = np.concatenate([lattice(), breakpoints()])
    keep = pred(a)
    bp = breakpoints()
    if real_pred is not None:           # the breakpoints' share of the count from the values, not from the bits
        with np.errstate(invalid="ignore"):
            bp_kept = int(real_pred(u2f(bp).astype(np.float64)).sum())
    elif domain == "no_snan":
        bp_kept = bp.size               # breakpoints() holds no NaN at all (neighbours() stops at the infinities)
        assert not is_nan(bp).any()
    else:
        bp_kept = bp.size
    b = np.concatenate([rotated(), np.roll(bp, 7)])[keep] if other_lane else None
    return Case(name, kind, a[keep], b, kept=lattice_kept + bp_kept, **kw)


def _binary(name, kind, **kw):
    """The lattice against its rotated copy, and the breakpoints against theirs."""
    bp = breakpoints()
    return Case(name, kind, np.concatenate([lattice(), bp]), np.concatenate([rotated(), np.roll(bp, 7)]), **kw)


def _pow():
    x = ((np.arange(65536, dtype=np.uint32)[:, None] << 16) | lower_halves()[None, :4]).reshape(-1)       # 2^16 by 4
    y = f2u(np.array([0.0, 1.0 / 2.2, 0.5, 1.0, 8.0, 64.0, -1.0, np.nan, np.inf], np.float32))
    return Case("det_pow", POW, np.repeat(x, y.size), np.tile(y, x.size), cap=0.505)


def _d24():
    stencil = np.random.default_rng(24).integers(0, 256, 1 << 24).astype(np.uint32) << 24
    return Case("d24_to_float", D24, np.arange(1 << 24, dtype=np.uint32) | stencil)


def _texel_index():
    """texel_index(fl, dim): the lattice without signaling NaNs, dim cycling through the sizes, and the breakpoints of every dim."""
    pred, lattice_kept, _ = DOMAINS["no_snan"]
    dims = np.array([2, 16, 130, 16384], np.uint32)
    a, b = lattice(), dims[np.arange(1 << 24) & 3]
    keep = pred(a)
    edge_a, edge_b = [], []
    for d in dims:
        n = neighbours([-2.0, -1.0, 0.0, float(d), float(d) + 1.0, 2.0 ** 31, -2.0 ** 31])
        edge_a.append(n); edge_b.append(np.full(n.size, d, np.uint32))
    ea, eb = np.concatenate(edge_a), np.concatenate(edge_b)
    return Case("texel_index", TEXEL_INDEX, np.concatenate([a[keep], ea]), np.concatenate([b[keep], eb]), kept=lattice_kept + ea.size, integer=True)


def _bilinear(s, o):
    """Output o of bilinear_setup<false>(u, v, w, h): the lattice against its rotated copy, and coordinates around the texel edges
    and centres of the first and last texels, the borders and both clamp ends."""
    w, h = SIZES[s]

    def edges(dim):
        i = np.concatenate([np.arange(-4, min(dim, 70) + 1), np.arange(max(dim - 70, 0), dim + 5)]).astype(np.float64)
        return neighbours(np.concatenate([i / dim, (i + 0.5) / dim]), 2)
    eu, ev = edges(w), edges(h)
    n = max(eu.size, ev.size)
    eu, ev = np.resize(eu, n), np.roll(np.resize(ev, n), 3)
    return Case("bilinear_setup[%dx%d].%s" % (w, h, ("i0", "j0", "fx", "fy")[o]), BILINEAR0 + 4 * s + o,
                np.concatenate([lattice(), eu, lattice()[:n]]), np.concatenate([rotated(), ev, ev]), integer=o < 2)


def _mul24():
    """Operands below 2^24 (the stated domain): the lattice's upper 24 bits against the rotated copy's, the edges crossed, and pairs
    with an operand above the domain, which the predicate must drop."""
    e = np.array([0, 1, 2, 0xFFF, 0x1000, 0x7FFFFF, 0x800000, 0xFFFFFE, 0xFFFFFF], np.uint32)
    a = np.concatenate([lattice() >> 8, np.repeat(e, e.size), np.array([1 << 24, 5, 0xFFFFFFFF], np.uint32)])
    b = np.concatenate([rotated() >> 8, np.tile(e, e.size), np.array([5, 1 << 24, 0xFFFFFFFF], np.uint32)])
    keep = (a < (1 << 24)) & (b < (1 << 24))
    return Case("mul24", MUL24, a[keep], b[keep], kept=(1 << 24) + e.size * e.size, integer=True)


# a result that is NaN when either of two independent lattice operands is: 2 x 0.39 % = 0.78 %, and 0 x inf, inf - inf and inf x 0
# on top (an infinite or zero operand is one lattice point in 2^15): 1 %
BINARY_CAP = 0.01

CASES = {
    # exhaustive
    "half_to_float": lambda: Case("half_to_float", HALF, np.arange(65536, dtype=np.uint32), cap=None),       # exhaustive: 2046 of the 65536 halves are NaN
    "unorm16_to_float": lambda: Case("unorm16_to_float", UNORM16, np.arange(65536, dtype=np.uint32)),
    "unorm8_to_float": lambda: Case("unorm8_to_float", UNORM8, np.arange(256, dtype=np.uint32)),
    "d24_to_float": _d24,
    # the lattice and the breakpoints
    "det_sin": lambda: _unary("det_sin", SIN),
    "det_cos": lambda: _unary("det_cos", COS),
    "det_log2": lambda: _unary("det_log2", LOG2, cap=0.505),
    "det_exp2": lambda: _unary("det_exp2", EXP2),
    "pow_inv_gamma": lambda: _unary("pow_inv_gamma", GAMMA, cap=0.505),
    "pow_inv_gamma2.y": lambda: _unary("pow_inv_gamma2.y", GAMMA2_Y, other_lane=True, cap=0.505),
    "pow_inv_gamma2.x": lambda: _unary("pow_inv_gamma2.x", GAMMA2_X, other_lane=True, cap=0.505),
    "rcp": lambda: _unary("rcp", RCP),
    "rcp_normal": lambda: _unary("rcp_normal", RCP_NORMAL, "rcp_normal"),
    "clamp_len2": lambda: _unary("clamp_len2", CLAMP_LEN2, "no_snan"),
    "sqrt_clamped": lambda: _unary("sqrt_clamped", SQRT_CLAMPED, "sqrt_clamped"),
    "len_from_sq": lambda: _unary("len_from_sq", LEN, "no_snan"),
    "inv_len_from_sq": lambda: _unary("inv_len_from_sq", INV_LEN, "no_snan"),
    "rcp2.x": lambda: _unary("rcp2.x", RCP2_X, other_lane=True),
    "rcp2.y": lambda: _unary("rcp2.y", RCP2_Y, other_lane=True),
    "rcp_normal2.x": lambda: _unary("rcp_normal2.x", RCP_NORMAL2_X, "rcp_normal", other_lane=True),
    "rcp_normal2.y": lambda: _unary("rcp_normal2.y", RCP_NORMAL2_Y, "rcp_normal", other_lane=True),
    "inv_len_from_sq2.x": lambda: _unary("inv_len_from_sq2.x", INV_LEN2_X, "no_snan", other_lane=True),
    "inv_len_from_sq2.y": lambda: _unary("inv_len_from_sq2.y", INV_LEN2_Y, "no_snan", other_lane=True),
    "saturate": lambda: _unary("saturate", SATURATE),
    "sign1": lambda: _unary("sign1", SIGN1),
    "signf": lambda: _unary("signf", SIGNF),
    "float_to_unorm8": lambda: _unary("float_to_unorm8", TO_UNORM8, integer=True),
    "float_to_unorm16": lambda: _unary("float_to_unorm16", TO_UNORM16, integer=True),
    # two arguments
    "det_pow": _pow,
    "divf": lambda: _binary("divf", DIVF, cap=BINARY_CAP),
    "maxnn": lambda: _binary("maxnn", MAXNN),
    "lerpf(a,b,.)": lambda: _binary("lerpf(a,b,.)", LERP_AB, cap=BINARY_CAP),
    "lerpf(.,b,t)": lambda: _binary("lerpf(.,b,t)", LERP_BT, cap=BINARY_CAP),
    "texel_index": _texel_index,
    "mul24": _mul24,
}
for _s in range(4):
    for _o in range(4):
        CASES["bilinear_setup[%dx%d].%s" % (SIZES[_s] + (("i0", "j0", "fx", "fy")[_o],))] = functools.partial(_bilinear, _s, _o)

# the soak run (CRY_DEVMATH_FULL=1): every unary kind over all 2^32 patterns -- name: (domain, the packed form's other lane is fed)
UNARY_FULL = {"det_sin": (None, False), "det_cos": (None, False), "det_log2": (None, False), "det_exp2": (None, False),
              "pow_inv_gamma": (None, False), "pow_inv_gamma2.x": (None, True), "pow_inv_gamma2.y": (None, True),
              "rcp": (None, False), "rcp2.x": (None, True), "rcp2.y": (None, True),
              "rcp_normal": ("rcp_normal", False), "rcp_normal2.x": ("rcp_normal", True), "rcp_normal2.y": ("rcp_normal", True),
              "clamp_len2": ("no_snan", False), "sqrt_clamped": ("sqrt_clamped", False), "len_from_sq": ("no_snan", False),
              "inv_len_from_sq": ("no_snan", False), "inv_len_from_sq2.x": ("no_snan", True), "inv_len_from_sq2.y": ("no_snan", True),
              "saturate": (None, False), "sign1": (None, False), "signf": (None, False),
              "float_to_unorm8": (None, False), "float_to_unorm16": (None, False)}


def full_chunks(name):
    """(a, b) of the soak run of a unary kind: all 2^32 patterns in 256 chunks of 2^24, the kind's domain applied; b is the other
    lane's pattern (a rotated within the chunk) or None."""
    domain, other_lane = UNARY_FULL[name]
    for hi in range(256):
        a = np.arange(hi << 24, (hi + 1) << 24, dtype=np.uint32)
        a = a[DOMAINS[domain][0](a)]
        if a.size:
            yield u2f(a), (u2f(np.roll(a, 7919)) if other_lane else None)


def same_results(case, got, ref):
    """Bit equality; for a float result any NaN equals any NaN (fuzz_util.same_floats).  Returns the number of differing elements."""
    g, r = got.view(np.uint32), ref.view(np.uint32)
    if case.integer:
        return int((g != r).sum())
    gn, rn = is_nan(g), is_nan(r)
    return int(((gn != rn) | (~gn & (g != r))).sum())


def nan_share(ref):
    return float(is_nan(ref.view(np.uint32)).mean())


