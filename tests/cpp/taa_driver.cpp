// taa_driver.cpp -- CRYCHIC::SetTemporalAA through the C++ veneer (include/crychic/CRYCHIC.h): the application's built-in scene is drawn
// with the switch off (plain.bin = the back buffer), then on for five frames while the camera strafes; each frame k leaves what the
// pass read and wrote: in_k.bin (the jittered back buffer), depth_k.bin, mats_k.bin (InvViewProj of the frame's constants, the
// unjittered ViewProj of this frame and of the previous one, the jitter: 50 floats), taa_k.bin (the pass's buffer) and hist_k.bin
// (the history it wrote).  Then a resize to the same size (resized_*.bin: a reset frame again), the pass in front of the depth of
// field and the anti-aliasing (chain_*.bin), and off again (plain_again.bin).  Parameters outside their ranges must be refused, and
// a strip with the switch on must make Draw throw (tests/test_taa_veneer.py).
// Usage: taa_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include <cstring>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [](PostDriver& d) {
        CRYCHIC& app = d.app;
        const std::string& dir = d.dir;
        const UINT W = d.W, H = d.H;
        if (app.TemporalAA() || app.TemporalAABackBuffer()) { std::fprintf(stderr, "temporal anti-aliasing is on by default\n"); return 4; }
        auto record = [&](const std::string& tag) {
            d.grab(app.CurrentBackBuffer(), "in_" + tag + ".bin");
            d.grab(app.DepthStencilBuffer(), "depth_" + tag + ".bin");
            d.grab(app.TemporalAABackBuffer(), "taa_" + tag + ".bin");
            d.grab(app.TemporalAAHistory(), "hist_" + tag + ".bin");
            float m[50];
            std::memcpy(m, &app.mMainPassCB.InvViewProj, 64);
            std::memcpy(m + 16, app.TemporalAAViewProj(0), 64);
            std::memcpy(m + 32, app.TemporalAAViewProj(1), 64);
            std::memcpy(m + 48, app.TemporalAAJitter(), 8);
            dump(dir + "/mats_" + tag + ".bin", m, sizeof m);
        };
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");

        // parameters outside their ranges are refused and leave the switch as it was
        int refused = 0;
        for (int which = 0; which < 4; ++which) {
            crychic_taa_params bad;
            crychic_taa_default_params(&bad);
            if (which == 0) bad.blend = 0;
            if (which == 1) bad.blend = 257;
            if (which == 2) bad.flags = 4;
            if (which == 3) bad.reserved[4] = 1;
            try { app.SetTemporalAA(bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        }
        if (refused != 4 || app.TemporalAA() || app.TemporalAABackBuffer()) { std::fprintf(stderr, "a bad parameter was not refused\n"); return 5; }

        // five frames with a strafing camera; a caller's blend reaches the pass (tests/test_taa_veneer.py states the same value)
        crychic_taa_params quick;
        crychic_taa_default_params(&quick);
        quick.blend = 64;
        app.SetTemporalAA(quick);
        if (!app.TemporalAA() || !app.TemporalAABackBuffer()) { std::fprintf(stderr, "SetTemporalAA(params)\n"); return 6; }
        for (int k = 0; k < 5; ++k) {
            if (k >= 2) app.mCamera.Strafe(0.05f * (float)k);
            d.frame();
            record(std::to_string(k));
        }

        // a strip with the switch on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        d.gt.Tick(1.0f / 60.0f);
        app.Update(d.gt);
        try { app.Draw(d.gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 5) { std::fprintf(stderr, "a strip with temporal anti-aliasing on did not throw\n"); return 7; }
        app.SetWholeFrame();

        // a resize (to the same size): new history planes, a reset frame
        app.Resize(W, H);
        d.frame();
        record("resized");

        // in front of the depth of field and the anti-aliasing, with the defaults
        app.SetTemporalAA(true);
        app.SetDepthOfField(true);
        app.SetAntiAliasing(true);
        d.frame();
        record("chain");
        d.grab(app.DepthOfFieldBackBuffer(), "chain_dof.bin");
        d.grab(app.AntiAliasedBackBuffer(), "chain_aa.bin");
        app.SetAntiAliasing(false);
        app.SetDepthOfField(false);

        // off again
        app.SetTemporalAA(false);
        if (app.TemporalAA() || app.TemporalAABackBuffer()) { std::fprintf(stderr, "SetTemporalAA(false)\n"); return 9; }
        app.mCamera.Strafe(-0.05f * (2 + 3 + 4));
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("taa driver ok %ux%u\n", W, H);
        return 0;
    });
}
