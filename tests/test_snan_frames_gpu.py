"""Signaling NaNs in whole frames, device tier: crychic_ssao_compute and the lighting entries over tests/snan_frames.py's planes against
the oracle and the features' checkers (the frames and references of tests/test_snan_frames_host.py).  Bar: test_fuzz.py's -- AO and
RGBA8 bit-exact, radiance equal up to NaN payloads.  On the device a signaling NaN that reached v_med3_f32 (clamp_len2, texel_index)
or v_max_f32 (saturate) unquieted would come out as something else than the definition says: every path from a plane load to them
has to pass an arithmetic instruction first."""
import ctypes as C

import numpy as np
import pytest

import snan_frames
from test_gloss_gpu import _call, _dev_planes, _frames_equal, _to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built_lib):
    from crychic_renderer_amd import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("size", snan_frames.SIZES)
def test_signaling_nans_in_the_planes_on_the_device(built_lib, ctx, size):
    import torch
    import gbuffer_f16_lib as gf
    from crychic_renderer_amd import Crychic
    r = snan_frames.reference(size, built_lib)
    W, H, p, c, knobs = r["W"], r["H"], r["planes"], r["c"], r["knobs"]
    assert r["bite"] >= 1
    ndl, radius, sky = knobs["numDirLights"], knobs["pcfSearchRadius"], knobs["sky"]
    lib, check = built_lib.lib, built_lib.check
    dev = {k: _to_dev(ctx, v) for k, v in p.items()}
    app = Crychic(ctx, W, H, dev["randvec"], dev["cube"], shadow_dim=p["shadow"].shape[1])
    app.load_scene({**dev, "consts": c})
    st = C.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
    a0, a1, edge = app.mSsao.mAmbientMap0, app.mSsao.mAmbientMap1, app.mSsao.mEdge
    check(lib.crychic_ssao_compute(ctx.handle, C.byref(c.ssao_cb), C.c_void_p(dev["normal"].data_ptr()), C.c_void_p(dev["depth"].data_ptr()),
                                   C.c_void_p(dev["randvec"].data_ptr()), C.c_void_p(a0.data_ptr()), C.c_void_p(a1.data_ptr()),
                                   C.c_void_p(edge.data_ptr()), W, H, 2, 0, H // 2, st))
    torch.cuda.synchronize()
    assert np.array_equal(a0.cpu().numpy().view(np.uint16), r["ao"]), size

    def light(planes, cube, cube_dim, flags):
        """crychic_deferred_light with the ambient map the SSAO call above left."""
        o = torch.zeros((H, W, 4), dtype=torch.uint8, device=ctx.device)
        rad = torch.zeros((H, W, 4), dtype=torch.float32, device=ctx.device)
        d = {k: _to_dev(ctx, planes[k]) for k in ("g0", "g1", "g2")}
        dcube = _to_dev(ctx, cube)
        sh = (C.c_void_p * 4)(*[dev["shadow"][k].data_ptr() for k in range(4)])
        check(lib.crychic_deferred_light(ctx.handle, C.byref(c.pass_cb), C.c_void_p(d["g0"].data_ptr()), C.c_void_p(d["g1"].data_ptr()),
                                         C.c_void_p(d["g2"].data_ptr()), C.c_void_p(dev["depth"].data_ptr()), C.c_void_p(a0.data_ptr()), sh,
                                         p["shadow"].shape[1], C.c_void_p(dcube.data_ptr()), cube_dim, C.c_void_p(o.data_ptr()),
                                         C.c_void_p(rad.data_ptr()), W, H, 0, H, ndl, radius, flags, st))
        torch.cuda.synchronize()
        return o, rad

    cd = int(p["cube"].shape[1])
    out, rad = light(p, p["cube"], cd, sky)
    assert _frames_equal(out, rad, r["plain"]), ("plain", size)
    out, rad = light(p, r["chain_cube"], cd, sky | (r["chain_kw"]["cube_levels"] << 16))
    assert _frames_equal(out, rad, r["chain"]), ("derivative chain", size)
    rc, out, rad = _call(lib, ctx, "light", c.pass_cb, _dev_planes(ctx, r["spec_planes"]), W, H, r["spec_flags"], cd, ndl=ndl, radius=radius)
    check(rc)
    torch.cuda.synchronize()
    assert _frames_equal(out, rad, r["spec"]), ("gloss + SH + split-sum", size)
    out, rad = light(r["half_planes"], p["cube"], cd, sky | gf.ALL_F16)
    assert _frames_equal(out, rad, r["half"]), ("all-half mix", size)
