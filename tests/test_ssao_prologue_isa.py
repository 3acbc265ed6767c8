"""ssao_kernel's prologue makes ONE memory round trip before the sky exit and before the first tap pair, checked in the gfx950
assembly the product is built from: tools/ssao_prologue_isa.py on the benchmark instantiation, and on hand-written snippets that
show the checker bites.  CPU tier: hipcc cross-compiles without a device.  One device compile of kernels.hip per module."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import handoff_isa as hi  # noqa: E402
import ssao_prologue_isa as sp  # noqa: E402


@pytest.fixture(scope="module")
def kernel(tmp_path_factory):
    d = tmp_path_factory.mktemp("ssao_prologue_isa")
    text = hi.device_asm(os.path.join(ROOT, "crychic_renderer_amd", "csrc", "kernels.hip"), str(d / "kernels.s"))
    return hi.kernel_body(text, sp.BENCH_KERNEL)


def test_one_batch_to_the_sky_exit_and_to_the_tap_loop(kernel):
    """At most one dependent load batch on every path from the entry to an s_endpgm ahead of the tap loops (the sky exit) and to
    the first block of a tap loop; the sky shortcut's fallback loop is the one labelled exception."""
    assert sp.check_prologue(kernel) == []
    assert sp.batch_counts(kernel) == (1, 1)


def test_kernel_has_the_expected_shape(kernel):
    """What the check keys on is really there, so that it cannot pass on an empty cut: tap loops with 16-byte footprint loads, one
    fallback loop with one 4-byte load, the centre / random-vector / cell loads ahead of them, an exit."""
    bl, index = hi.blocks(kernel)
    taps, fallback, errors = sp.classify(kernel)
    assert errors == []
    assert len(taps) >= 2 and len(fallback) >= 1
    ahead = [s for i, (_, ins) in enumerate(bl) if i < min(taps) and i not in fallback for s in ins if sp.is_load(s)]
    count = lambda m: sum(1 for s in ahead if hi.mnemonic(s) == m)
    assert count("global_load_dwordx2") >= 3          # two depth pairs and the normal texel (+ the two border texels)
    assert count("global_load_dword") >= 5            # four random-vector texels and the geometry-map cell
    assert any(s.startswith("s_endpgm") for _, ins in bl for s in ins)
    assert any(sp.vm_wait(s) is not None for _, ins in bl for s in ins)


# ---- the checker itself, on hand-written assembly -----------------------------------------------------------------------------
# A miniature of the kernel: the batch, the stores, the sky vote with its fallback loop and exit, the tap loop, the tail.

BATCH = """
    s_cbranch_execz .Lend
    global_load_dwordx2 v[4:5], v4, s[16:17]
    global_load_dwordx2 v[10:11], v9, s[18:19]
    global_load_dword v16, v20, s[8:9]
    s_cbranch_vccnz .Lnocell
    global_load_dword v20, v[20:21], off
.Lnocell:
    s_and_saveexec_b64 s[4:5], vcc
    s_cbranch_execz .Lnoborder
    global_load_dwordx2 v[24:25], v[24:25], off
.Lnoborder:
    s_or_b64 exec, exec, s[4:5]
"""
RESOLVE = """
    s_waitcnt vmcnt(3)
    v_cvt_f32_u32_e32 v1, v10
    s_waitcnt vmcnt(0)
    global_store_dwordx2 v[28:29], v[4:5], off
"""
SKY = """
    s_cbranch_vccnz .Llit
    s_cbranch_scc0 .Lvote
.Lfallback:
    global_load_dword v6, v[12:13], off
    s_waitcnt vmcnt(0)
    s_cbranch_execnz .Lfallback
.Lvote:
    s_cbranch_vccnz .Llit
    global_store_short v[6:7], v3, off
    s_endpgm
.Llit:
"""
TAPS = """
.Ltaps:
    global_load_dword v60, v59, s[26:27]
    s_waitcnt vmcnt(0)
    global_load_dwordx4 v[66:69], v61, s[20:21]
    s_waitcnt vmcnt(0)
    s_cbranch_scc1 .Ltaps
    global_store_short v[6:7], v3, off
.Lend:
    s_endpgm
"""


def check(text):
    return sp.check_prologue(text.splitlines())


def test_snippet_one_batch_passes():
    assert check(BATCH + RESOLVE + SKY + TAPS) == []
    assert sp.batch_counts((BATCH + RESOLVE + SKY + TAPS).splitlines()) == (1, 1)
    assert check(BATCH + RESOLVE.replace("vmcnt(0)", "0") + SKY + TAPS) == []           # the all-zero immediate waits too


def test_snippet_reload_after_the_wait_fails():
    """The shape before the change: the normal texel loaded again behind the centre's wait, ahead of the stores."""
    bad = RESOLVE.replace("    global_store", "    global_load_dwordx2 v[16:17], v[16:17], off\n    s_waitcnt vmcnt(0)\n    global_store")
    errs = check(BATCH + bad + SKY + TAPS)
    assert "an exit ahead of the tap loop is reachable after 2 dependent load batches (limit 1)" in errs
    assert "a tap loop is reachable after 2 dependent load batches (limit 1)" in errs


def test_snippet_load_behind_a_partial_wait_fails():
    """vmcnt(3) with loads outstanding is a wait like any other: what is issued behind it could not go out with the batch."""
    bad = RESOLVE.replace("    v_cvt_f32_u32_e32 v1, v10\n", "    global_load_dword v17, v21, s[8:9]\n")
    assert any("2 dependent load batches" in e for e in check(BATCH + bad + SKY + TAPS))


def test_snippet_random_vector_loads_on_the_lit_path_fail():
    """The shape before the change: the random-vector texels fetched behind the sky vote.  The sky exit is fine, the tap loop is not."""
    errs = check(BATCH + RESOLVE + SKY + "    global_load_dword v13, v12, s[50:51]\n    s_waitcnt vmcnt(0)\n" + TAPS)
    assert errs == ["a tap loop is reachable after 2 dependent load batches (limit 1)"]


def test_snippet_border_copy_on_one_arm_fails():
    """A load-wait-store in a branch of its own: one path suffices."""
    bad = RESOLVE + "    s_and_saveexec_b64 s[4:5], vcc\n    s_cbranch_execz .Lskip\n    global_load_dwordx2 v[6:7], v[6:7], off offset:8\n" \
        "    s_waitcnt vmcnt(0)\n    global_store_dwordx2 v[8:9], v[6:7], off\n.Lskip:\n"
    assert any("exit ahead of the tap loop is reachable after 2" in e for e in check(BATCH + bad + SKY + TAPS))


def test_snippet_fallback_loop_is_the_only_exception():
    # a second load in the fallback loop
    two = SKY.replace("    global_load_dword v6, v[12:13], off\n", "    global_load_dword v6, v[12:13], off\n    global_load_dword v7, v[14:15], off\n")
    assert any("fallback loop holds more than one" in e for e in check(BATCH + RESOLVE + two + TAPS))
    # a second load-wait loop ahead of the tap loop
    other = "\n.Lother:\n    global_load_dword v8, v[12:13], off\n    s_waitcnt vmcnt(0)\n    s_cbranch_execnz .Lother\n"
    assert any("only the sky shortcut's fallback is an exception" in e for e in check(BATCH + RESOLVE + SKY + other + TAPS))
    # a cell load behind the vote, outside the loop, is a batch like any other
    late = SKY.replace(".Lvote:\n", ".Lvote:\n    global_load_dword v6, v[12:13], off\n    s_waitcnt vmcnt(0)\n")
    assert any("exit ahead of the tap loop is reachable after 2" in e for e in check(BATCH + RESOLVE + late + TAPS))


def test_snippet_without_a_tap_loop_is_refused():
    assert any("no tap loop found" in e for e in check(BATCH + RESOLVE + SKY + "    s_endpgm\n.Lend:\n    s_endpgm\n"))
    assert check("") == ["empty kernel body"]
