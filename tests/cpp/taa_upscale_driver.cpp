// taa_upscale_driver.cpp -- CRYCHIC::SetTemporalUpscale through the C++ veneer (include/crychic/CRYCHIC.h): the application's built-in
// scene is drawn with the switch off (plain.bin = the back buffer), then on at 3/2 of the client size for four frames while the camera
// strafes; each frame k leaves what the pass read and wrote: in_k.bin (the jittered back buffer), depth_k.bin, mats_k.bin (InvViewProj
// of the frame's constants, the unjittered ViewProj of this frame and of the previous one, the jitter: 50 floats), up_k.bin (the pass's
// buffer) and hist_k.bin (the history it wrote).  Then a resize to the same size (resized_*.bin: a reset frame again), the bloom and
// the anti-aliasing behind the pass at the display size (chain_*.bin, and final.ppm from Present), and off again (plain_again.bin).
// Parameters and sizes outside their ranges must be refused; a strip, and the temporal anti-aliasing, the depth of field or the motion
// blur together with the switch, must make Draw throw (tests/test_taa_upscale_veneer.py).
// Usage: taa_upscale_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include <cstring>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [](PostDriver& d) {
        CRYCHIC& app = d.app;
        const std::string& dir = d.dir;
        const UINT W = d.W, H = d.H, WO = W * 3 / 2, HO = H * 3 / 2;
        if (app.TemporalUpscale() || app.TemporalUpscaleBackBuffer() || app.FinalWidth() != W || app.FinalHeight() != H) {
            std::fprintf(stderr, "temporal upsampling is on by default\n");
            return 4;
        }
        auto record = [&](const std::string& tag) {
            d.grab(app.CurrentBackBuffer(), "in_" + tag + ".bin");
            d.grab(app.DepthStencilBuffer(), "depth_" + tag + ".bin");
            d.grab(app.TemporalUpscaleBackBuffer(), "up_" + tag + ".bin");
            d.grab(app.TemporalUpscaleHistory(), "hist_" + tag + ".bin");
            float m[50];
            std::memcpy(m, &app.mMainPassCB.InvViewProj, 64);
            std::memcpy(m + 16, app.TemporalAAViewProj(0), 64);
            std::memcpy(m + 32, app.TemporalAAViewProj(1), 64);
            std::memcpy(m + 48, app.TemporalAAJitter(), 8);
            dump(dir + "/mats_" + tag + ".bin", m, sizeof m);
        };
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");

        // parameters and sizes outside their ranges are refused and leave the switch as it was
        int refused = 0;
        for (int which = 0; which < 8; ++which) {
            crychic_taa_upscale_params bad;
            crychic_taa_upscale_default_params(&bad);
            UINT w = WO, h = HO;
            if (which == 0) bad.blend = 0;
            if (which == 1) bad.blend = 257;
            if (which == 2) bad.flags = 4;
            if (which == 3) bad.reserved[4] = 1;
            if (which == 4) w = W - 1;
            if (which == 5) w = 4 * W + 1;
            if (which == 6) h = H - 1;
            if (which == 7) h = 4 * H + 1;
            try { app.SetTemporalUpscale(w, h, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        }
        if (refused != 8 || app.TemporalUpscale() || app.TemporalUpscaleBackBuffer()) { std::fprintf(stderr, "a bad parameter was not refused\n"); return 5; }

        // four frames with a strafing camera; a caller's blend reaches the pass (tests/test_taa_upscale_veneer.py states the same value)
        crychic_taa_upscale_params quick;
        crychic_taa_upscale_default_params(&quick);
        quick.blend = 200;
        app.SetTemporalUpscale(WO, HO, &quick);
        if (!app.TemporalUpscale() || !app.TemporalUpscaleBackBuffer() || app.FinalWidth() != WO || app.FinalHeight() != HO) {
            std::fprintf(stderr, "SetTemporalUpscale(params)\n");
            return 6;
        }
        for (int k = 0; k < 4; ++k) {
            if (k >= 2) app.mCamera.Strafe(0.05f * (float)k);
            d.frame();
            record(std::to_string(k));
        }

        // a strip with the switch on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        d.gt.Tick(1.0f / 60.0f);
        app.Update(d.gt);
        try { app.Draw(d.gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        app.SetWholeFrame();
        // the three stages that cannot stand with it
        for (int which = 0; which < 3; ++which) {
            if (which == 0) app.SetTemporalAA(true);
            if (which == 1) app.SetDepthOfField(true);
            if (which == 2) app.SetMotionBlur(true);
            try { app.Draw(d.gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
            if (which == 0) app.SetTemporalAA(false);
            if (which == 1) app.SetDepthOfField(false);
            if (which == 2) app.SetMotionBlur(false);
        }
        if (refused != 12) { std::fprintf(stderr, "a refusal of Draw is missing (%d)\n", refused); return 7; }

        // a resize (to the same size): new history planes, a reset frame
        app.Resize(W, H);
        d.frame();
        record("resized");

        // the bloom and the anti-aliasing behind it, at the display size, with the pass's defaults
        app.SetTemporalUpscale(WO, HO);
        app.SetBloom(true);
        app.SetAntiAliasing(true);
        d.frame();
        record("chain");
        d.grab(app.BloomBackBuffer(), "chain_bloom.bin");
        d.grab(app.AntiAliasedBackBuffer(), "chain_aa.bin");
        app.Present(dir + "/final.ppm");
        app.SetAntiAliasing(false);
        app.SetBloom(false);

        // off again
        app.SetTemporalUpscale(0, 0);
        if (app.TemporalUpscale() || app.TemporalUpscaleBackBuffer() || app.FinalWidth() != W) { std::fprintf(stderr, "SetTemporalUpscale(0, 0)\n"); return 9; }
        app.mCamera.Strafe(-0.05f * (2 + 3));
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("taa upscale driver ok %ux%u -> %ux%u\n", W, H, WO, HO);
        return 0;
    });
}
