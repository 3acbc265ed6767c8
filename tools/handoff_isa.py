"""Path-sensitive check of the blur chain's tile hand-off in the gfx950 assembly the product is built from.

    python tools/handoff_isa.py            # compiles csrc/kernels.hip with build.FLAGS, checks blur_replay_chain_kernel

blur_replay_chain_kernel (csrc/kernels.hip) is the one place where workgroups hand data to each other inside a launch: a
tile's workgroup stores its texels, publishes a per-tile counter, and its neighbours poll the counter and read the texels.
Whether that is ordered is decided by the instructions the compiler emitted, not by the source, so this tool reads the
assembly: it cuts the kernel's body out, splits it into basic blocks and runs forward may-analyses over the control-flow
graph (loops included; the order of lines in the file proves nothing).

Producer, three bits per wavefront:
    D  a payload store (global_store_short) may still be un-drained            set by the store, cleared by s_waitcnt vmcnt(0)
    N  a payload store was issued and no s_barrier has been passed since        set by the store, cleared by s_barrier
    B  the wavefront may have passed its latest s_barrier with D set            s_barrier copies D into B
At the signal (the sc1 global_store_dwordx2 of the progress counter) all three must be clear on every path: every storing
wavefront drained its stores, THEN reached the workgroup barrier, and only then one lane publishes.  The plain
global_store_dwordx2 is the timeout word of the bounded poll's give-up path and signals nothing.

Consumer (the agent-scope acquire is kept), one state per wavefront and path:
    clean -> polled (global_load_dwordx2) -> invalidated (buffer_inv sc1) -> waited (s_waitcnt vmcnt(0)) -> clean (s_barrier)
Every global_load_ushort (a handed-off texel) must be reached in state clean only.

tests/test_chain_handoff_isa.py runs these checks on the real kernel and on hand-written snippets that must fail.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_KERNEL = "blur_replay_chain_kernel"

PAYLOAD_STORE = "global_store_short"
PAYLOAD_LOAD = "global_load_ushort"
COUNTER_STORE = "global_store_dwordx2"
POLL_LOAD = "global_load_dwordx2"


def device_asm(source, out_path, hipcc=None):
    """gfx950 assembly of one .hip source with the flags the product is built with (crychic_renderer_amd/build.py FLAGS)."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from crychic_renderer_amd import build
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [hipcc or os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + flags + ["--cuda-device-only", "-S", "-I", os.path.join(ROOT, "include"),
                                                                                "-I", build.CSRC, "-x", "hip", source, "-o", out_path]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out_path) as f:
        return f.read()


def functions(text):
    """-> {symbol: [lines of its body]} for every function of an assembly file (label ... .Lfunc_endN)."""
    out, name, body, typed = {}, None, [], set()
    for raw in text.splitlines():
        m = re.match(r"^\s*\.type\s+([\w$.]+),@function", raw)
        if m:
            typed.add(m.group(1))
        if name is None:
            m = re.match(r"^([A-Za-z_$][\w$.]*):", raw)
            if m and m.group(1) in typed:
                name, body = m.group(1), []
        elif re.match(r"^\.Lfunc_end\d+:", raw):
            out[name] = body
            name = None
        else:
            body.append(raw)
    return out


def kernel_body(text, name_part):
    hits = [(n, b) for n, b in functions(text).items() if name_part in n]
    if len(hits) != 1:
        raise LookupError("%d functions match %r" % (len(hits), name_part))
    return hits[0][1]


def instructions(lines):
    """Labels ('name:') and instructions of a body, comments and directives dropped, white space normalised."""
    out = []
    for raw in lines:
        s = " ".join(raw.split(";")[0].split())
        if not s:
            continue
        if re.match(r"^[.\w$]+:$", s):
            out.append(s)
        elif not s.startswith("."):
            out.append(s)
    return out


def blocks(lines):
    """-> (basic blocks [(label or None, [instruction, ...])], label -> block index): cut at labels and after branches / s_endpgm."""
    out, cur, lab = [], [], None
    for s in instructions(lines):
        if s.endswith(":") and " " not in s:
            if cur or lab is not None:
                out.append((lab, cur))
            lab, cur = s[:-1], []
            continue
        cur.append(s)
        if s.startswith(("s_branch", "s_cbranch", "s_endpgm")):
            out.append((lab, cur))
            lab, cur = None, []
    if cur or lab is not None:
        out.append((lab, cur))
    return out, {l: i for i, (l, _) in enumerate(out) if l is not None}


def successors(bl, index, i):
    ins = bl[i][1]
    last = ins[-1] if ins else ""
    if last.startswith("s_endpgm"):
        return []
    if last.startswith("s_branch"):
        return [index[last.split()[1]]]
    nxt = [i + 1] if i + 1 < len(bl) else []
    if last.startswith("s_cbranch"):
        return nxt + [index[last.split()[1]]]
    return nxt


def mnemonic(s):
    return s.split()[0]


def has_sc1(s):
    return "sc1" in s.split()[1:]


def drains_vm(s):
    return mnemonic(s) == "s_waitcnt" and ("vmcnt(0)" in s or re.fullmatch(r"s_waitcnt 0(x0+)?", s) is not None)


def dataflow(lines, start, step, join):
    """Forward may-analysis to a fixed point.  step(state, instruction, report) -> state; join(a, b) -> state."""
    bl, index = blocks(lines)
    errors = []
    if not bl:
        return ["empty kernel body"]
    IN = [None] * len(bl)
    IN[0] = start
    work = [0]
    while work:
        i = work.pop()
        state = IN[i]
        for s in bl[i][1]:
            state = step(state, s, errors.append)
        for j in successors(bl, index, i):
            new = state if IN[j] is None else join(IN[j], state)
            if new != IN[j]:
                IN[j] = new
                work.append(j)
    return errors


def check_producer(lines):
    """Checks 1 - 3: sc1 payload stores; drain, then barrier, then signal on every path; sc1 counter store and poll."""
    ins = [s for s in instructions(lines) if not s.endswith(":")]
    errors = []
    for s in ins:
        m = mnemonic(s)
        if m == PAYLOAD_STORE and not has_sc1(s):
            errors.append("payload store without sc1: " + s)
        if m == POLL_LOAD and not has_sc1(s):
            errors.append("poll load without sc1: " + s)
        if m.startswith(("global_atomic", "buffer_atomic", "buffer_store", "flat_", "scratch_")):
            errors.append("access the hand-off's checker has no rule for: " + s)
    if not any(mnemonic(s) == PAYLOAD_STORE for s in ins):
        errors.append("no payload store found")
    if not any(mnemonic(s) == POLL_LOAD for s in ins):
        errors.append("no poll load found")
    if not any(mnemonic(s) == COUNTER_STORE and has_sc1(s) for s in ins):
        errors.append("no signal store found (an sc1 %s)" % COUNTER_STORE)

    def step(state, s, report):
        D, N, B = state
        m = mnemonic(s)
        if m == PAYLOAD_STORE:
            D = N = True
        elif drains_vm(s):
            D = False
        elif m == "s_barrier":
            B, N = D, False
        elif m == COUNTER_STORE and has_sc1(s):
            if D or B:
                report("signal store reachable with an un-drained payload store (D=%s, B=%s)" % (D, B))
            if N:
                report("signal store reachable with no s_barrier after a payload store (another wavefront's stores may be in flight)")
        return (D, N, B)

    errors += dataflow(lines, (False, False, False), step, lambda a, b: tuple(x or y for x, y in zip(a, b)))
    return sorted(set(errors))


CLEAN, POLLED, INVALIDATED, WAITED = 1, 2, 4, 8
_STATE_NAMES = {POLLED: "no buffer_inv sc1 after the poll", INVALIDATED: "no s_waitcnt vmcnt(0) after the buffer_inv sc1",
                WAITED: "no s_barrier after the acquire's wait"}


def check_consumer_acquire(lines):
    """Check 4 with the acquire kept: sc1 texel loads, no flat access, and poll -> buffer_inv sc1 -> s_waitcnt vmcnt(0) -> s_barrier
    on every path from the poll to a texel load."""
    ins = [s for s in instructions(lines) if not s.endswith(":")]
    errors = []
    for s in ins:
        if mnemonic(s) == PAYLOAD_LOAD and not has_sc1(s):
            errors.append("payload load without sc1: " + s)
        if mnemonic(s).startswith("flat_"):
            errors.append("flat access: " + s)
    if not any(mnemonic(s) == PAYLOAD_LOAD for s in ins):
        errors.append("no payload load found")
    if not any(mnemonic(s) == "buffer_inv" and has_sc1(s) for s in ins):
        errors.append("no agent-scope acquire (buffer_inv sc1) found")

    def move(states, frm, to):
        return (states & ~frm) | to if states & frm else states

    def step(states, s, report):
        m = mnemonic(s)
        if m == POLL_LOAD:
            states = POLLED
        elif m == "buffer_inv" and has_sc1(s):
            states = move(states, POLLED, INVALIDATED)
        elif drains_vm(s):
            states = move(states, INVALIDATED, WAITED)
        elif m == "s_barrier":
            states = move(states, WAITED, CLEAN)
        elif m == PAYLOAD_LOAD:
            for bit, what in _STATE_NAMES.items():
                if states & bit:
                    report("payload load reachable from the poll with " + what)
        return states

    errors += dataflow(lines, CLEAN, step, lambda a, b: a | b)
    return sorted(set(errors))


def check_handoff(lines):
    return check_producer(lines) + check_consumer_acquire(lines)


def kernels_containing(text, mnem):
    """Names of the functions of an assembly file whose body holds an instruction with this mnemonic."""
    return sorted(n for n, b in functions(text).items() if any(mnemonic(s) == mnem for s in instructions(b) if not s.endswith(":")))


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        if len(sys.argv) > 1:
            with open(sys.argv[1]) as f:
                text = f.read()
        else:
            text = device_asm(os.path.join(ROOT, "crychic_renderer_amd", "csrc", "kernels.hip"), os.path.join(d, "kernels.s"))
    errs = check_handoff(kernel_body(text, CHAIN_KERNEL))
    print("\n".join(errs) if errs else "OK")
    sys.exit(1 if errs else 0)
