// motion_blur_driver.cpp -- CRYCHIC::SetMotionBlur through the C++ veneer (include/crychic/CRYCHIC.h): the application's built-in scene
// is drawn with the switch off (plain.bin = the back buffer), then on for five frames while the camera strafes from the third on; each
// frame k leaves what the pass read and wrote: in_k.bin (the back buffer), depth_k.bin, mats_k.bin (InvViewProj of the frame's
// constants, the unjittered ViewProj of this frame and of the previous one: 48 floats), mb_k.bin (the pass's buffer) and ws_k.bin (its
// workspace).  Then a resize to the same size (resized_*.bin: no previous camera again), the pass behind the depth of field and in front
// of the bloom and the anti-aliasing (chain_*.bin), and off again (plain_again.bin).  Parameters outside their ranges must be refused,
// and a strip with the switch on must make Draw throw (tests/test_motion_blur_veneer.py).
// Usage: motion_blur_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include <cstring>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [](PostDriver& d) {
        CRYCHIC& app = d.app;
        const std::string& dir = d.dir;
        const UINT W = d.W, H = d.H;
        if (app.MotionBlur() || app.MotionBlurBackBuffer() || app.MotionBlurWorkspace()) { std::fprintf(stderr, "motion blur is on by default\n"); return 4; }
        auto record = [&](const std::string& tag) {
            d.grab(app.CurrentBackBuffer(), "in_" + tag + ".bin");
            d.grab(app.DepthStencilBuffer(), "depth_" + tag + ".bin");
            d.grab(app.MotionBlurBackBuffer(), "mb_" + tag + ".bin");
            d.grab(app.MotionBlurWorkspace(), "ws_" + tag + ".bin");
            float m[48];
            std::memcpy(m, &app.mMainPassCB.InvViewProj, 64);
            std::memcpy(m + 16, app.MotionBlurViewProj(0), 64);
            std::memcpy(m + 32, app.MotionBlurViewProj(1), 64);
            dump(dir + "/mats_" + tag + ".bin", m, sizeof m);
        };
        const DirectX::XMFLOAT3 home = app.mCamera.GetPosition3f();
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");

        // parameters outside their ranges are refused and leave the switch as it was
        int refused = 0;
        for (int which = 0; which < 6; ++which) {
            crychic_motion_blur_params bad;
            crychic_motion_blur_default_params(&bad);
            if (which == 0) bad.shutter = 257;
            if (which == 1) bad.samples = 6;
            if (which == 2) bad.samples = 64;
            if (which == 3) bad.maxRadius = 0;
            if (which == 4) bad.flags = 1;
            if (which == 5) bad.reserved[2] = 1;
            try { app.SetMotionBlur(true, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        }
        if (refused != 6 || app.MotionBlur() || app.MotionBlurBackBuffer()) { std::fprintf(stderr, "a bad parameter was not refused\n"); return 5; }

        // five frames; the camera strafes from the third on; a caller's parameters reach the pass (tests/test_motion_blur_veneer.py states them)
        crychic_motion_blur_params wide;
        crychic_motion_blur_default_params(&wide);
        wide.shutter = 256;
        wide.samples = 16;
        wide.maxRadius = 24;
        app.SetMotionBlur(true, &wide);
        if (!app.MotionBlur() || !app.MotionBlurBackBuffer() || !app.MotionBlurWorkspace()) { std::fprintf(stderr, "SetMotionBlur(params)\n"); return 6; }
        for (int k = 0; k < 5; ++k) {
            if (k >= 2) app.mCamera.Strafe(0.15f * (float)k);
            d.frame();
            record(std::to_string(k));
        }

        // a strip with the switch on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        d.gt.Tick(1.0f / 60.0f);
        app.Update(d.gt);
        try { app.Draw(d.gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 7) { std::fprintf(stderr, "a strip with motion blur on did not throw\n"); return 7; }
        app.SetWholeFrame();

        // a resize (to the same size): the next frame has no previous camera, although the camera moves
        app.Resize(W, H);
        app.mCamera.Strafe(0.3f);
        d.frame();
        record("resized");

        // behind the depth of field, in front of the bloom and the anti-aliasing, with the defaults
        app.SetMotionBlur(true);
        app.SetDepthOfField(true);
        app.SetBloom(true);
        app.SetAntiAliasing(true);
        app.mCamera.Strafe(0.4f);
        d.frame();
        record("chain");
        d.grab(app.DepthOfFieldBackBuffer(), "chain_dof.bin");
        d.grab(app.BloomBackBuffer(), "chain_bloom.bin");
        d.grab(app.AntiAliasedBackBuffer(), "chain_aa.bin");
        app.SetAntiAliasing(false);
        app.SetBloom(false);
        app.SetDepthOfField(false);

        // off again
        app.SetMotionBlur(false);
        if (app.MotionBlur() || app.MotionBlurBackBuffer() || app.MotionBlurWorkspace()) { std::fprintf(stderr, "SetMotionBlur(false)\n"); return 9; }
        app.mCamera.SetPosition(home.x, home.y, home.z);
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("motion blur driver ok %ux%u\n", W, H);
        return 0;
    });
}
