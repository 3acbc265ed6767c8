"""The wave votes of the lighting kernels on the device (DESIGN.md section 3 "wave votes"): every frame of the corpus of
tests/light_votes_lib.py -- whose wavefronts tests/test_light_votes_host.py::test_census shows to be unanimous, refused by exactly
one lane at each end and in the middle of the wavefront, partial, and unanimous over uncovered lanes that hold the spoiler, for
every vote a configuration reaches -- through crychic_deferred_light == the oracle, and through crychic_deferred_light_point_shadows
(40 point lights and 8 spot lights, 2 of each shadowed) and with the gloss lookup, SH ambient and the split-sum table over G1 and G2
as half4 (the general family) == those families' checkers: RGBA8 byte for byte, radiance by bits (NaN ==
NaN: fuzz_util.same_floats), tolerance none.  Each configuration as the whole frame and as three row ranges; guard bytes around
both outputs and the rows outside a range must come back untouched."""
import ctypes as C

import numpy as np
import pytest

import fuzz_util
import light_votes_lib as lv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GUARD_ROWS = 4
FILL = 0xA5


@pytest.fixture(scope="module")
def ctx(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected but no HIP device is visible")
    from crychic_renderer_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def device_corpus(ctx):
    """The corpus on the device, uploaded once."""
    co = lv.corpus()

    def dev(a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else (a.view(np.int16) if a.dtype == np.uint16 else a)).to(ctx.device)
    frames = []
    for fr in co.frames:
        d = {k: dev(fr.planes[k]) for k in ("g0", "g1", "g2", "depth", "shadow")}
        d["ambient"] = dev(fr.ambient)
        half = lv.planes_of(fr, [c for c in lv.CONFIGS if c.family == "general"][0])[0]
        d["g1 half"], d["g2 half"] = dev(half["g1"]), dev(half["g2"])
        frames.append(d)
    return co, frames, {"cube": dev(co.cube), "chain": dev(co.chain), "general": dev(lv.general_call())}


@pytest.mark.parametrize("cfg", lv.CONFIGS, ids=[c.name for c in lv.CONFIGS])
def test_device_equals_oracle_over_the_corpus(ctx, built_lib, oracle, device_corpus, cfg):
    lib, check = built_lib.lib, built_lib.check
    co, frames, cubes = device_corpus
    W, H, G = lv.W, lv.H, GUARD_ROWS
    general = cfg.family == "general"
    cube = cubes["general" if general else ("chain" if cfg.chain else "cube")]
    flags = cfg.flags | (lv.HALF_G1_G2 if general else 0)
    g1, g2 = ("g1 half", "g2 half") if general else ("g1", "g2")
    P = lambda t: C.c_void_p(t.data_ptr())
    out = torch.empty((H + 2 * G, W, 4), dtype=torch.uint8, device=ctx.device)
    rad = torch.empty((H + 2 * G, W, 4), dtype=torch.float32, device=ctx.device)
    local = cfg.family == "point shadows"
    if local:
        from local_lights_util import dev_lights
        from point_shadow_lib import point_desc, spot_desc
        lo = lv.local_lights()
        (dp, n_points), (ds, n_spots) = dev_lights(ctx, lo["points"]), dev_lights(ctx, lo["spots"])
        dmaps = torch.from_numpy(lo["maps"].view(np.int32)).to(ctx.device)
        dcubes = torch.from_numpy(lo["cubes"].view(np.int32)).to(ctx.device)
        sdesc, pdesc = spot_desc(dmaps), point_desc(dcubes, lo["projs"])
    for k, d in enumerate(frames):
        shadow_ptrs = (C.c_void_p * 4)(*[d["shadow"][i].data_ptr() for i in range(4)])
        for row0, rows in lv.ROW_RANGES:
            out.fill_(FILL); rad.view(torch.uint8).fill_(FILL)
            args = [P(d["g0"]), P(d[g1]), P(d[g2]), P(d["depth"]), P(d["ambient"]), shadow_ptrs, lv.SHADOW_DIM, P(cube), lv.CUBE_DIM,
                    P(out[G]), P(rad[G]), W, H, row0, rows, lv.NUM_DIR_LIGHTS, cfg.radius, flags]
            if local:
                check(lib.crychic_deferred_light_point_shadows(ctx.handle, C.byref(lo["cb"]), *args, P(dp), n_points, P(ds), n_spots,
                                                               C.byref(sdesc), C.byref(pdesc), None))
            else:
                check(lib.crychic_deferred_light(ctx.handle, C.byref(co.cb), *args, None))
            torch.cuda.synchronize()
            got, got_rad = out.cpu().numpy(), rad.cpu().numpy()
            where = (co.frames[k].name, row0, rows)
            ref, ref_rad = lv.reference(oracle, k, cfg, row0, rows)
            inside = np.zeros(H + 2 * G, bool); inside[G + row0:G + row0 + rows] = True
            assert (got[~inside] == FILL).all(), ("RGBA8 written outside the rows", where)
            assert (got_rad[~inside].view(np.uint8) == FILL).all(), ("radiance written outside the rows", where)
            sel = slice(row0, row0 + rows)
            assert np.array_equal(got[G:G + H][sel], ref[sel]), (where, int((got[G:G + H][sel] != ref[sel]).sum()))
            assert fuzz_util.same_floats(got_rad[G:G + H][sel], ref_rad[sel]), where


def test_no_call_splits_a_quad(ctx, built_lib, device_corpus):
    """Vote 13's remaining case -- a quad split by the end of a call -- cannot reach a kernel: every lighting entry refuses an odd frame
    height, and with the derivative chain an odd row0 and an odd row count (which an even height can never end the frame with)."""
    lib = built_lib.lib
    co, frames, cubes = device_corpus
    cfg, d = lv.chain_config(), frames[0]
    P = lambda t: C.c_void_p(t.data_ptr())
    out = torch.full((lv.H, lv.W, 4), FILL, dtype=torch.uint8, device=ctx.device)
    shadow_ptrs = (C.c_void_p * 4)(*[d["shadow"][i].data_ptr() for i in range(4)])

    def call(h, row0, rows):
        return lib.crychic_deferred_light(ctx.handle, C.byref(co.cb), P(d["g0"]), P(d["g1"]), P(d["g2"]), P(d["depth"]), P(d["ambient"]), shadow_ptrs,
                                          lv.SHADOW_DIM, P(cubes["chain"]), lv.CUBE_DIM, P(out), None, lv.W, h, row0, rows, lv.NUM_DIR_LIGHTS,
                                          cfg.radius, cfg.flags, None)
    assert call(63, 0, 63) == -1 and b"even" in lib.crychic_last_error()
    assert call(63, 42, 21) == -1
    assert call(lv.H, 42, 21) == -1 and b"whole pixel quads" in lib.crychic_last_error()
    assert call(lv.H, 43, 21) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == FILL).all()                    # the refused calls enqueued nothing
