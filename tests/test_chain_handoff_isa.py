"""The blur chain's tile hand-off (kernels.hip blur_replay_chain_kernel), checked in the gfx950 assembly the product is built
from: tools/handoff_isa.py on the real kernel, and on hand-written snippets that show the checker bites.  CPU tier: hipcc
cross-compiles without a device.  One device compile of kernels.hip and one of raster.hip per module."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import handoff_isa as hi  # noqa: E402


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("handoff_isa")
    csrc = os.path.join(ROOT, "crychic_renderer_amd", "csrc")
    from concurrent.futures import ThreadPoolExecutor
    names = ("kernels", "raster")
    with ThreadPoolExecutor(2) as pool:         # the two compiles side by side
        return dict(zip(names, pool.map(lambda n: hi.device_asm(os.path.join(csrc, n + ".hip"), str(d / (n + ".s"))), names)))


@pytest.fixture(scope="module")
def chain(device_asm):
    return hi.kernel_body(device_asm["kernels"], hi.CHAIN_KERNEL)


def test_chain_kernel_publishes_after_drain_and_barrier(chain):
    """Checks 1 - 3: every texel store is write-through (sc1); on every path to the progress counter's store every wavefront has
    executed s_waitcnt vmcnt(0) after its texel stores and then passed the workgroup barrier; counter store and poll are sc1."""
    assert hi.check_producer(chain) == []


def test_chain_kernel_acquires_before_it_stages(chain):
    """Check 4, the acquire kept: every texel load is an sc1 global load, there is no flat access, and on every path from the poll
    to a texel load lie buffer_inv sc1, s_waitcnt vmcnt(0) and s_barrier, in this order."""
    assert hi.check_consumer_acquire(chain) == []


def test_chain_kernel_has_the_expected_accesses(chain):
    """What the checks key on is really there, so that they cannot pass on an empty cut."""
    ins = [s for s in hi.instructions(chain) if not s.endswith(":")]
    count = lambda m, sc1: sum(1 for s in ins if hi.mnemonic(s) == m and hi.has_sc1(s) == sc1)
    assert count("global_store_short", True) >= 1 and count("global_store_short", False) == 0
    assert count("global_load_ushort", True) >= 8 and count("global_load_ushort", False) == 0
    assert count("global_store_dwordx2", True) == 1           # the progress counter
    assert count("global_store_dwordx2", False) == 1          # the timeout word of the give-up path
    assert count("global_load_dwordx2", True) == 1 and count("global_load_dwordx2", False) == 0
    assert sum(1 for s in ins if hi.mnemonic(s) == "s_barrier") >= 3
    assert any(s.startswith("s_endpgm") for s in ins)


def test_no_other_kernel_polls(device_asm):
    """Tripwire: the chain's poll is the only s_sleep of the library.  A second in-launch hand-off needs a checker entry of its
    own here before it can ship."""
    assert [n for n in hi.kernels_containing(device_asm["kernels"], "s_sleep") if hi.CHAIN_KERNEL not in n] == []
    assert len(hi.kernels_containing(device_asm["kernels"], "s_sleep")) == 1
    assert hi.kernels_containing(device_asm["raster"], "s_sleep") == []
    assert len(hi.functions(device_asm["kernels"])) > 5 and len(hi.functions(device_asm["raster"])) > 3


# ---- the checker itself, on hand-written assembly -----------------------------------------------------------------------------
# A miniature of the kernel: a bounded poll with its give-up store, a barrier, a loop of texel loads and stores, the tail.

HEAD = """
    s_cbranch_execz .Lstage
.Lpoll:
    global_load_dwordx2 v[6:7], v[2:3], off sc1
    s_waitcnt vmcnt(0)
    v_cmp_eq_u32_e32 vcc, v6, v8
    s_cbranch_vccnz .Lmatched
    s_sleep 16
    s_add_i32 s9, s9, -1
    s_cmp_lg_u32 s9, 0
    s_cbranch_scc1 .Lpoll
    global_store_dwordx2 v1, v[2:3], s[6:7]
.Lmatched:
    s_waitcnt vmcnt(0) lgkmcnt(0)
    buffer_inv sc1
    s_waitcnt vmcnt(0)
.Lstage:
    s_barrier
    global_load_ushort v39, v[22:23], off sc1
    s_waitcnt vmcnt(0)
    s_barrier
"""
SIGNAL = """
    s_and_saveexec_b64 s[0:1], vcc
    s_cbranch_execz .Lend
    global_store_dwordx2 v2, v[0:1], s[0:1] sc1
.Lend:
    s_endpgm
"""
STORE_LOOP = """
.Lrows:
    global_store_short v[10:11], v8, off sc1
    s_add_i32 s4, s4, 1
    s_cmp_lt_u32 s4, s5
    s_cbranch_scc1 .Lrows
"""


def producer(text):
    return hi.check_producer((HEAD + text + SIGNAL).splitlines())


def test_snippet_drain_barrier_signal_passes():
    assert producer(STORE_LOOP + "s_waitcnt vmcnt(0)\n s_barrier\n") == []
    assert producer(STORE_LOOP + "s_waitcnt 0\n s_barrier\n") == []                      # the all-zero immediate drains too
    assert hi.check_consumer_acquire((HEAD + STORE_LOOP + "s_waitcnt vmcnt(0)\n s_barrier\n" + SIGNAL).splitlines()) == []


def test_snippet_no_wait_fails():
    """The shape before the fix: an LDS-only wait and the barrier."""
    errs = producer(STORE_LOOP + "s_waitcnt lgkmcnt(0)\n s_barrier\n")
    assert errs == ["signal store reachable with an un-drained payload store (D=True, B=True)"]


def test_snippet_wait_on_one_arm_fails():
    errs = producer(STORE_LOOP + "s_cbranch_scc0 .Lskip\n s_waitcnt vmcnt(0)\n.Lskip:\n s_barrier\n")
    assert any("un-drained" in e for e in errs)


def test_snippet_wait_before_store_in_loop_fails():
    """The wait sits in the loop body ahead of the store: the last store of the loop leaves by the back edge un-drained."""
    loop = """
.Lrows:
    s_waitcnt vmcnt(0)
    global_store_short v[10:11], v8, off sc1
    s_add_i32 s4, s4, 1
    s_cmp_lt_u32 s4, s5
    s_cbranch_scc1 .Lrows
"""
    assert any("un-drained" in e for e in producer(loop + "s_barrier\n"))
    # ... while a wait behind the store inside the loop does drain every store
    assert producer(loop.replace("    s_waitcnt vmcnt(0)\n    global_store_short v[10:11], v8, off sc1\n",
                                 "    global_store_short v[10:11], v8, off sc1\n    s_waitcnt vmcnt(0)\n") + "s_barrier\n") == []


def test_snippet_wait_without_barrier_fails():
    """Every wavefront drains its own stores, but nothing holds the signalling lane until the OTHER wavefronts have."""
    errs = producer(STORE_LOOP + "s_waitcnt vmcnt(0)\n")
    assert errs == ["signal store reachable with no s_barrier after a payload store (another wavefront's stores may be in flight)"]
    # the barrier ahead of the wait is no better: a wavefront passes it with stores in flight
    assert any("B=True" in e for e in producer(STORE_LOOP + "s_barrier\n s_waitcnt vmcnt(0)\n"))


def test_snippet_missing_sc1_fails():
    good = HEAD + STORE_LOOP + "s_waitcnt vmcnt(0)\n s_barrier\n" + SIGNAL
    assert any("payload store without sc1" in e for e in hi.check_producer(good.replace("v8, off sc1", "v8, off").splitlines()))
    assert any("poll load without sc1" in e for e in hi.check_producer(good.replace("v[2:3], off sc1", "v[2:3], off").splitlines()))
    assert any("no signal store" in e for e in hi.check_producer(good.replace("s[0:1] sc1", "s[0:1]").splitlines()))
    assert any("payload load without sc1" in e for e in hi.check_consumer_acquire(good.replace("v[22:23], off sc1", "v[22:23], off").splitlines()))
    assert any("flat access" in e for e in hi.check_consumer_acquire(good.replace("global_load_ushort v39, v[22:23], off", "flat_load_ushort v39, v[22:23]").splitlines()))


def test_snippet_consumer_forms_fail():
    good = HEAD + STORE_LOOP + "s_waitcnt vmcnt(0)\n s_barrier\n" + SIGNAL
    consumer = lambda t: hi.check_consumer_acquire(t.splitlines())
    assert consumer(good) == []
    # no acquire at all (the shape before the fix)
    errs = consumer(good.replace("    buffer_inv sc1\n", ""))
    assert "payload load reachable from the poll with no buffer_inv sc1 after the poll" in errs
    # a workgroup-scope invalidate is not the acquire
    assert any("no buffer_inv sc1" in e for e in consumer(good.replace("buffer_inv sc1", "buffer_inv sc0")))
    # the acquire only on the give-up path: the matched exit of the loop skips it
    moved = good.replace("    buffer_inv sc1\n", "").replace("    global_store_dwordx2 v1, v[2:3], s[6:7]\n", "    global_store_dwordx2 v1, v[2:3], s[6:7]\n    buffer_inv sc1\n")
    assert any("no buffer_inv sc1" in e for e in consumer(moved))
    # the invalidate not waited for before the barrier releases the other wavefronts
    assert any("no s_waitcnt vmcnt(0) after the buffer_inv" in e for e in consumer(good.replace("    buffer_inv sc1\n    s_waitcnt vmcnt(0)\n", "    buffer_inv sc1\n")))
    # no barrier between the acquire and the loads
    assert any("no s_barrier after the acquire" in e for e in consumer(good.replace(".Lstage:\n    s_barrier\n", ".Lstage:\n")))
