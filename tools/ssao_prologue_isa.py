"""Counts the dependent load batches of ssao_kernel's prologue in the gfx950 assembly the product is built from.

    python tools/ssao_prologue_isa.py            # compiles csrc/kernels.hip with build.FLAGS, checks ssao_kernel<1,1,1,0>

A sky wavefront of ssao_kernel (csrc/kernels.hip) does no arithmetic to speak of: its life is the number of memory round trips
it makes one after the other.  A lit wavefront pays the same trips before its first tap pair.  The kernel therefore issues
everything its prologue reads -- centre depth and normal, the random-vector texels, the geometry-map cell of the sky shortcut,
the border texels of the edge workspace -- as ONE batch before it waits for any of it.  Whether it really does is decided by
the instructions the compiler emitted, so this tool reads the assembly, with the block / dataflow machinery of handoff_isa.py.

A "batch" is a run of global loads that no wait separates: a global_load_* issued after an s_waitcnt with a vmcnt field that
had loads outstanding opens a new one (it could not be issued before something else had come back).  The forward may-analysis
carries, per path, (batches so far, loads outstanding, a wait has been passed since the last load was issued) and reports the
largest batch count with which
    * an s_endpgm is reached without entering the tap loop (the sky exit, and the exit of the lanes outside the frame), and
    * a tap loop is entered.
Both must be at most one.  Loops are the cycles of the control-flow graph: one that holds a global_load_dwordx4 (the tap
footprints) is a tap loop, and the prologue ends where one is entered; the one other loop with a load is the sky shortcut's
fallback for a rectangle of more cells than the wavefront has lanes, the labelled exception: its loads are not counted, and it
may hold nothing but one global_load_dword.

The tool looks at loads, waits and branches and at nothing else.  tests/test_ssao_prologue_isa.py runs it on the real kernel and
on hand-written snippets that must fail.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handoff_isa as hi  # noqa: E402

BENCH_KERNEL = "ssao_kernelILb1ELb1ELb1ELb0E"      # ssao_kernel<EMIT_AO, PAIRS, MAPS, !ROWS>: what the benchmark frame runs
TAP_LOAD = "global_load_dwordx4"
CAP = 6                                            # batch counts saturate here (the analysis must terminate on loops)


def is_load(s):
    return hi.mnemonic(s).startswith("global_load_")


def vm_wait(s):
    """None: not a wait on the vector-memory counter; otherwise the count it waits down to."""
    if hi.mnemonic(s) != "s_waitcnt":
        return None
    m = re.search(r"vmcnt\((\d+)\)", s)
    if m:
        return int(m.group(1))
    if re.fullmatch(r"s_waitcnt 0(x0+)?", s):
        return 0
    return None


def loops(bl, index):
    """-> the loops of the control-flow graph as sets of blocks: its strongly connected components with an edge inside (a loop
    nest is one component).  A backward branch to a shared exit block is on no cycle and is no loop."""
    n = len(bl)
    succ = [hi.successors(bl, index, i) for i in range(n)]
    reach = []
    for i in range(n):
        seen, work = set(), list(succ[i])
        while work:
            j = work.pop()
            if j not in seen:
                seen.add(j)
                work.extend(succ[j])
        reach.append(seen)
    out, done = [], set()
    for i in range(n):
        if i in done or i not in reach[i]:
            continue
        comp = frozenset(j for j in reach[i] if i in reach[j])
        done |= comp
        out.append(comp)
    return out


def classify(lines):
    """-> (blocks of the tap loops, blocks of the fallback loop, errors)."""
    bl, index = hi.blocks(lines)
    taps, fallback, errors = set(), set(), []
    nfallback = 0
    for comp in loops(bl, index):
        loads = [s for i in sorted(comp) for s in bl[i][1] if is_load(s)]
        if any(hi.mnemonic(s) == TAP_LOAD for s in loads):
            taps |= comp
        elif loads:
            nfallback += 1
            if len(loads) != 1 or hi.mnemonic(loads[0]) != "global_load_dword":
                errors.append("the fallback loop holds more than one global_load_dword: " + "; ".join(loads))
            fallback |= comp
    if not taps:
        errors.append("no tap loop found (a loop with a %s)" % TAP_LOAD)
    if nfallback > 1:
        errors.append("%d loops with loads ahead of the tap loops: only the sky shortcut's fallback is an exception" % nfallback)
    return taps, fallback, errors


def check_prologue(lines, limit=1):
    """Errors of the kernel body `lines`: more than `limit` dependent load batches on a path to an exit or to a tap-loop header."""
    bl, index = hi.blocks(lines)
    if not bl:
        return ["empty kernel body"]
    taps, fallback, errors = classify(lines)
    if not any(s.startswith("s_endpgm") for _, ins in bl for s in ins):
        errors.append("no s_endpgm found")

    # state: frozenset of (batches, outstanding, waited) -- one entry per distinguishable path
    def step_one(st, s, exempt):
        b, out, waited = st
        if is_load(s):
            if exempt:
                return (b, out, waited)
            if b == 0 or waited:
                b = min(b + 1, CAP)
            return (b, True, False)
        w = vm_wait(s)
        if w is not None and out:
            return (b, w > 0, True)
        return st

    IN = [None] * len(bl)
    IN[0] = frozenset([(0, False, False)])
    work = [0]
    worst_exit, worst_tap = 0, 0
    while work:
        i = work.pop()
        states = IN[i]
        if i in taps:                                  # the prologue ends here
            continue
        for s in bl[i][1]:
            states = frozenset(step_one(st, s, i in fallback) for st in states)
        for j in hi.successors(bl, index, i):
            new = states if IN[j] is None else IN[j] | states
            if new != IN[j]:
                IN[j] = new
                work.append(j)
    for i, (_, ins) in enumerate(bl):
        if IN[i] is None:
            continue
        if i in taps:
            worst_tap = max(worst_tap, max(b for b, _, _ in IN[i]))
        elif ins and ins[-1].startswith("s_endpgm"):
            states = IN[i]
            for s in ins:
                states = frozenset(step_one(st, s, i in fallback) for st in states)
            worst_exit = max(worst_exit, max(b for b, _, _ in states))
    if taps and all(IN[h] is None for h in taps):
        errors.append("no tap loop is reachable from the entry")
    if worst_exit > limit:
        errors.append("an exit ahead of the tap loop is reachable after %d dependent load batches (limit %d)" % (worst_exit, limit))
    if worst_tap > limit:
        errors.append("a tap loop is reachable after %d dependent load batches (limit %d)" % (worst_tap, limit))
    return sorted(set(errors))


def batch_counts(lines):
    """(largest batch count at an exit ahead of the tap loop, at a tap-loop header) -- for reports."""
    worst = [0, 0]
    for limit in range(CAP + 1):
        errs = check_prologue(lines, limit)
        if not any("exit ahead" in e for e in errs) and worst[0] == 0:
            worst[0] = limit
        if not any("a tap loop is reachable after" in e for e in errs) and worst[1] == 0:
            worst[1] = limit
        if worst[0] and worst[1]:
            break
    return tuple(worst)


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        if len(sys.argv) > 1:
            with open(sys.argv[1]) as f:
                text = f.read()
        else:
            text = hi.device_asm(os.path.join(hi.ROOT, "crychic_renderer_amd", "csrc", "kernels.hip"), os.path.join(d, "kernels.s"))
    body = hi.kernel_body(text, BENCH_KERNEL)
    errs = check_prologue(body)
    print("dependent load batches: %d to the sky exit, %d to the tap loop" % batch_counts(body))
    print("\n".join(errs) if errs else "OK")
    sys.exit(1 if errs else 0)
