"""The depth-of-field pass against a lens-sampled ground truth (a script, not a test).

    python tests/dof_quality.py [--size 320x180] [--samples 48] [--focus 15] [--apertures 6,3,12]

The reference scene on the CPU (crychic_renderer_amd.scene's ray caster, the oracle's SSAO and lighting pass) from --samples points
on a lens disc (a Vogel spiral): the ray of a pixel starts at the lens point and goes through the point the pinhole ray of that pixel
meets at the focus distance, so the plane in focus stays fixed and everything else shears; the frames are averaged as RGBA8.  The lens
radius that matches `aperture` pixels is aperture * focus * tan(fovY / 2) / (H / 2).  Reports, for each aperture, the mean absolute
RGBA8 error against that ground truth of the plain (pinhole) frame and of the checker's output (tests/dof_ref) over the plain frame,
and the same over the pixels the pass changes.  The sky and the view vector of the specular term are the pinhole's in every sample
(InvViewProj and the G-buffer layout are per pixel, not per lens point); EyePosW follows the lens point.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def lens_planes(scene, consts, off, focus):
    """The normal / depth / G-buffer planes of scene._camera_planes for rays that start `off` = (dx, dy) from the eye on the lens and
    pass through the pinhole ray's point at distance `focus` along the view axis (dx = dy = 0: the pinhole frame)."""
    import torch
    W, H, cam = consts.W, consts.H, consts.cam
    dt, dev = torch.float64, torch.device("cpu")
    eye = torch.tensor(list(cam.pos), dtype=dt)
    R, U, L = scene._camera_basis(cam, dev, dt)
    th = math.tan(0.5 * cam.fovY)
    xs = (torch.arange(W, dtype=dt) + 0.5) / W * 2.0 - 1.0
    ys = 1.0 - (torch.arange(H, dtype=dt) + 0.5) / H * 2.0
    vx = (xs * cam.aspect * th)[None, :].expand(H, W).reshape(-1)
    vy = (ys * th)[:, None].expand(H, W).reshape(-1)
    shift = off[0] * R + off[1] * U
    D = vx[:, None] * R[None] + vy[:, None] * U[None] + L[None] - shift[None] / focus       # still one unit along L
    O = (eye + shift)[None].expand_as(D).contiguous()
    t, nrm, mat = scene.raycast(O, D)
    hit = torch.isfinite(t)
    tt = torch.where(hit, t, torch.zeros_like(t))
    pos = O + tt[:, None] * D
    A = cam.farZ / (cam.farZ - cam.nearZ)
    B = -cam.nearZ * cam.farZ / (cam.farZ - cam.nearZ)
    zndc = A + B / torch.where(hit, tt, torch.ones_like(tt))
    d24 = torch.round(zndc.clamp(0.0, 1.0) * 16777215.0).to(torch.int64)
    d24 = torch.where(hit & (tt >= cam.nearZ) & (tt <= cam.farZ), d24, torch.full_like(d24, 0xFFFFFF))
    covered = d24 < 0xFFFFFF
    nview = torch.stack([nrm @ R, nrm @ U, nrm @ L], dim=1)
    normal = torch.zeros((H * W, 4), dtype=torch.float32)
    normal[:, 2] = 1.0
    normal[covered, :3] = nview[covered].to(torch.float32)
    base = torch.ones((H * W, 3), dtype=dt)
    base[mat == 1] = 0.9
    rough = torch.full((H * W,), 0.8, dtype=dt)
    rough[mat == 0] = 0.3
    rough[mat == 1] = 0.7
    tex = 0.75 + 0.25 * torch.sin(3.1 * pos[:, 0] + 1.7 * pos[:, 1]) * torch.cos(2.3 * pos[:, 2] - 0.9 * pos[:, 1])
    albedo = base * torch.stack([tex, 0.9 * tex + 0.1, 0.8 * tex + 0.2], dim=1)
    bump = 0.12 * torch.stack([torch.sin(9.0 * pos[:, 0] + 4.0 * pos[:, 2]), torch.sin(7.0 * pos[:, 1]),
                               torch.cos(8.0 * pos[:, 2] - 3.0 * pos[:, 0])], dim=1)
    nW = nrm + bump * (1.0 - nrm.abs())
    g0, g1, g2 = (torch.zeros((H * W, 4), dtype=torch.float32) for _ in range(3))
    g0[covered, :3] = pos[covered].to(torch.float32)
    g0[covered, 3] = 0.5
    g1[covered, :3] = albedo[covered].to(torch.float32)
    g1[covered, 3] = rough[covered].to(torch.float32)
    g2[covered, :3] = nW[covered].to(torch.float32)
    g2[covered, 3] = 1.0
    return {"depth": d24.to(torch.int32).reshape(H, W).numpy().view(np.uint32), "normal": normal.to(torch.float16).reshape(H, W, 4).numpy(),
            "g0": g0.reshape(H, W, 4).numpy(), "g1": g1.reshape(H, W, 4).numpy(), "g2": g2.reshape(H, W, 4).numpy()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="320x180")
    ap.add_argument("--samples", type=int, default=48)
    ap.add_argument("--focus", type=float, default=15.0)
    ap.add_argument("--apertures", default="6,3,12")
    ap.add_argument("--shadow-dim", type=int, default=1024)
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    import dof_lib as dl
    import oracle_lib
    from crychic_renderer_amd import lib, scene
    consts = scene.Constants(W, H, a.shadow_dim)
    shared = scene.make_scene(W, H, shadow_dim=a.shadow_dim, cube_dim=64, device="cpu", consts=consts)
    shadow, cube, randvec = shared["shadow"].numpy().view(np.uint32), shared["cube"].numpy(), shared["randvec"].numpy()
    orc = oracle_lib.load()
    scb = oracle_lib.as_oracle_cb(consts.ssao_cb, oracle_lib.OrSsaoConstants)
    pcf = lib.crychic_pcf_search_radius(a.shadow_dim, 1)
    R, U, _ = scene._camera_basis(consts.cam, "cpu", __import__("torch").float64)

    def shade(off):
        p = lens_planes(scene, consts, off, a.focus)
        pcb = oracle_lib.as_oracle_cb(consts.pass_cb, oracle_lib.OrPassConstants)
        moved = np.array(list(consts.cam.pos)) + off[0] * R.numpy() + off[1] * U.numpy()
        f = np.frombuffer((C.c_char * C.sizeof(pcb)).from_address(C.addressof(pcb)), np.float32)
        f[304:307] = moved                                          # EyePosW (tests/fog_lib.py has the offset)
        ao = orc.compute_ssao(scb, p["normal"], p["depth"], randvec, 3)
        return orc.deferred_light(pcb, p["g0"], p["g1"], p["g2"], p["depth"], ao, shadow, cube, 3, pcf, sky=True), p["depth"]

    plain, depth = shade((0.0, 0.0))
    frame = dl.Frame.from_pass_cb(consts.pass_cb, depth)
    out = {"metric": "dof_quality", "frame": [W, H], "samples": a.samples, "focus": a.focus}
    th = math.tan(0.5 * consts.cam.fovY)
    for ap_px in (float(v) for v in a.apertures.split(",")):
        radius = ap_px * a.focus * th / (0.5 * H)
        acc = np.zeros((H, W, 4), np.float64)
        for i in range(a.samples):
            r, phi = radius * math.sqrt((i + 0.5) / a.samples), i * 2.399963229728653
            acc += shade((r * math.cos(phi), r * math.sin(phi)))[0]
        truth = acc / a.samples
        got = dl.checker(frame, plain, dict(focus=a.focus, aperture=ap_px, radius=8))[0].astype(np.float64)
        changed = (got != plain).any(-1)
        tag = "ap%g" % ap_px
        out[tag + "_lens_radius"] = round(radius, 4)
        out[tag + "_mae_plain"] = round(float(np.abs(plain - truth).mean()), 4)
        out[tag + "_mae_pass"] = round(float(np.abs(got - truth).mean()), 4)
        out[tag + "_changed_share"] = round(float(changed.mean()), 4)
        out[tag + "_mae_plain_changed"] = round(float(np.abs(plain - truth)[changed].mean()), 4)
        out[tag + "_mae_pass_changed"] = round(float(np.abs(got - truth)[changed].mean()), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
