"""What the motion blur does to the picture (recorded in profiles/motion_blur_quality.txt, README.md and DESIGN.md section 25, not a
test):

    python tests/motion_blur_quality.py [--size 320x180] [--poses 16] [--shadow-dim 512] [--out profiles/motion_blur_quality.txt]

The reference scene lit by the CPU oracle (blurCount 3, 3 lights, sky, --shadow-dim cascades, literal PCF radius) at --size under two
cameras: one that strafes 0.6 world units a frame and one that turns 0.06 rad a frame.  The ground truth of a frame is the rounded mean
of --poses oracle frames at poses interpolated (position and yaw, linearly) over the exposure interval, shutter / 256 of the frame
interval, centred on the current pose.  The current frame goes through the checker of crychic_motion_blur (tests/motion_blur_ref: the
definition the device reproduces byte for byte) with the previous pose's view-projection, at the default shutter and radius and N = 4,
8 and 16.  Prints one JSON line per camera: the mean absolute RGBA8 error against the truth of the unblurred frame and of the pass."""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="320x180")
    ap.add_argument("--poses", type=int, default=16)
    ap.add_argument("--shadow-dim", type=int, default=512)
    ap.add_argument("--out", default="", help="also write the JSON lines to this file")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.lower().split("x"))
    import motion_blur_lib as mbl
    import oracle_lib
    import scene_util
    from crychic_renderer_amd import lib, scene
    orc = oracle_lib.load()
    base = scene.make_scene(W, H, shadow_dim=a.shadow_dim, cube_dim=64, device="cpu")

    def frame(cam):
        """(lit frame, depth plane, InvViewProj, ViewProj) of the scene seen by `cam`."""
        consts = scene.Constants(W, H, a.shadow_dim, cam=cam)
        p = scene_util.np_planes(dict(base, **scene._camera_planes(consts, "cpu")))
        scb = oracle_lib.as_oracle_cb(consts.ssao_cb, oracle_lib.OrSsaoConstants)
        pcb = oracle_lib.as_oracle_cb(consts.pass_cb, oracle_lib.OrPassConstants)
        ao = orc.compute_ssao(scb, p["normal"], p["depth"], p["randvec"], 3)
        lit = orc.deferred_light(pcb, p["g0"], p["g1"], p["g2"], p["depth"], ao, p["shadow"], p["cube"], 3, lib.crychic_pcf_search_radius(a.shadow_dim, 1),
                                 sky=True)
        return (np.ascontiguousarray(lit), np.ascontiguousarray(p["depth"]), np.array(consts.pass_cb.InvViewProj[:], np.float32),
                np.array(consts.pass_cb.ViewProj[:], np.float32))

    lines = []
    for name, step in (("strafe", dict(dx=0.6)), ("turn", dict(yaw=0.06))):
        def pose(t):        # t frames after the current pose; the previous pose is t = -1
            return mbl.moved_camera(W, H, **{k: v * t for k, v in step.items()})
        plain, depth, ivp, cur = frame(pose(0.0))
        prev = frame(pose(-1.0))[3]
        sh = mbl.DEFAULT_SHUTTER / 256.0
        total = np.zeros(plain.shape, np.int64)
        for j in range(a.poses):
            total += frame(pose(sh * ((j + 0.5) / a.poses - 0.5)))[0]
        truth = (2 * total + a.poses) // (2 * a.poses)

        def mae(img):
            return round(float(np.abs(img.astype(np.int64) - truth).mean()), 5)
        out = {"camera": name, "step": step, "size": [W, H], "poses": a.poses, "shutter": mbl.DEFAULT_SHUTTER, "maxRadius": mbl.DEFAULT_RADIUS,
               "mae_unblurred": mae(plain)}
        for n in (4, 8, 16):
            case = mbl.Case("%s_n%d" % (name, n), ivp, cur, prev, depth, plain, samples=n)
            ws, branch = mbl.checker_velocity(case)
            blurred = mbl.checker_gather(case, ws, branch=branch)
            out["mae_n%d" % n] = mae(blurred)
            if n == 8:
                words = mbl.velocity_words(ws, W, H)[0]
                length = np.maximum(np.abs((words & 0xFFFF).astype(np.int16)), np.abs((words >> 16).astype(np.int16)))
                out["mean_velocity_px"] = round(float(length.mean()) / 16.0, 3)
                out["pixels_changed_share"] = round(float((blurred != plain).any(-1).mean()), 4)
                out["clamped_share"] = round(float(((branch & mbl.B_CLAMPED) != 0).mean()), 4)
        out["lowers_the_error"] = all(out["mae_n%d" % n] < out["mae_unblurred"] for n in (4, 8, 16))
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
