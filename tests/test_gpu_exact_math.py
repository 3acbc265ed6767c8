"""The exact reciprocal / square-root / inverse-length sequences of csrc/devmath.hpp against their definitions, for EVERY
binary32 bit pattern, on the GPU (tools/exact_math_probe.hip: v_rcp_f32 / v_sqrt_f32 / v_rsq_f32 + one correction step vs the
IEEE expansions the compiler emits for `1.0f / x` and `sqrtf(x)`).  The hardware seeds are not reproducible on a CPU, so this
is where the claim "the device path equals the oracle's or_rcp / or_len / or_inv_len" is established; the parity tests then
check the whole kernels.  The packed forms the SSAO tap loop runs (rcp2, rcp_normal2, inv_len_from_sq2: each lane, the other lane
fed a rotated pattern) and rcp_normal are swept as well, the *_normal ones over every pattern of their stated domain
2^-126 <= |b| <= 2^126.  The probe is built with the product's flag set."""
import re
import subprocess

import pytest

import devmath_dev_lib

ALL = ("rcp (devmath.hpp) vs or_rcp", "len_from_sq vs or_len", "inv_len_from_sq vs or_inv_len", "rcp2.x vs or_rcp", "rcp2.y vs or_rcp",
       "inv_len_from_sq2.x vs or_inv_len", "inv_len_from_sq2.y vs or_inv_len")                    # rows that cover all 2^32 patterns
DOMAIN = ("rcp_normal vs or_rcp", "rcp_normal2.x vs or_rcp", "rcp_normal2.y vs or_rcp")          # rows that cover the domain
DOMAIN_PATTERNS = 2 * (0x7E800001 - 0x00800000)            # exponent fields 1 .. 252 and 2^126 itself, both signs


def build_probe():
    return devmath_dev_lib.build_probe()


def test_probe_compiles():
    import os
    assert os.path.exists(build_probe())


@pytest.mark.gpu
def test_shipped_sequences_equal_their_definitions_exhaustively():
    r = subprocess.run([build_probe(), "shipped"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = re.findall(r"^(\S.*?)\s+inputs \[([0-9a-f]{8,9}), ([0-9a-f]{8,9})\): (\d+) differ", r.stdout, flags=re.M)
    names = {n.strip() for n, *_ in rows}
    assert set(ALL) | set(DOMAIN) <= names, r.stdout
    covered = dict.fromkeys(names, 0)
    for name, lo, hi, bad in rows:
        assert int(bad) == 0, (name, lo, hi, bad)
        covered[name.strip()] += int(hi, 16) - int(lo, 16)
    for name in ALL:
        assert covered[name] == 1 << 32, (name, covered[name])              # every bit pattern
    for name in DOMAIN:
        assert covered[name] == DOMAIN_PATTERNS, (name, covered[name])      # every pattern of the stated domain
