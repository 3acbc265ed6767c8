// sharpen_driver.cpp -- CRYCHIC::SetSharpening through the C++ veneer (include/crychic/CRYCHIC.h): the application's built-in scene is
// drawn with the stage off (plain.bin = the back buffer), then with it on at the defaults (sharp_frame.bin = the back buffer, sharp.bin
// = the stage's buffer), behind the temporal anti-aliasing with other parameters (sharp_taa_in.bin = the resolved frame the stage
// read, sharp_taa.bin), behind the temporal upsampling at the display size with the anti-aliasing behind it (sharp_up_in.bin,
// sharp_up.bin, sharp_up_aa.bin), then off again (plain_again.bin); what is refused must leave the stage as it was, and a strip with
// it on must make Draw throw (tests/test_sharpen_veneer.py).
// Usage: sharpen_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights> <WO> <HO>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [&](PostDriver& d) {
        CRYCHIC& app = d.app;
        const UINT H = d.H, WO = std::atoi(argv[8]), HO = std::atoi(argv[9]);
        if (app.Sharpening() || app.SharpenedBackBuffer()) { std::fprintf(stderr, "the sharpening is on by default\n"); return 4; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");

        app.SetSharpening(true);
        if (!app.Sharpening() || !app.SharpenedBackBuffer()) { std::fprintf(stderr, "SetSharpening\n"); return 5; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "sharp_frame.bin");
        d.grab(app.SharpenedBackBuffer(), "sharp.bin");

        // what is refused leaves the stage as it was
        int refused = 0;
        crychic_sharpen_params bad;
        crychic_sharpen_default_params(&bad);
        bad.strength = CRYCHIC_SHARPEN_MAX_STRENGTH + 1;
        try { app.SetSharpening(true, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        crychic_sharpen_default_params(&bad);
        bad.limit = CRYCHIC_SHARPEN_MAX_LIMIT + 1;
        try { app.SetSharpening(true, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        crychic_sharpen_default_params(&bad);
        bad.reserved[1] = 1;
        try { app.SetSharpening(false, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 3 || !app.Sharpening()) { std::fprintf(stderr, "bad parameters were not refused\n"); return 6; }
        d.frame();
        d.grab(app.SharpenedBackBuffer(), "sharp_again.bin");

        // a strip with the stage on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        d.gt.Tick(1.0f / 60.0f);
        app.Update(d.gt);
        try { app.Draw(d.gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG && std::string(e.what()).find("sharpening") != std::string::npos; }
        if (refused != 4) { std::fprintf(stderr, "a strip with the sharpening on did not throw, or did not name it\n"); return 7; }
        app.SetWholeFrame();

        // behind the temporal anti-aliasing, with the whole of the widest limit
        crychic_sharpen_params strong;
        crychic_sharpen_default_params(&strong);
        strong.strength = CRYCHIC_SHARPEN_MAX_STRENGTH; strong.limit = CRYCHIC_SHARPEN_MAX_LIMIT;
        app.SetSharpening(true, &strong);
        app.SetTemporalAA(true);
        d.frame();
        d.frame();
        d.grab(app.TemporalAABackBuffer(), "sharp_taa_in.bin");
        d.grab(app.SharpenedBackBuffer(), "sharp_taa.bin");
        app.SetTemporalAA(false);

        // behind the temporal upsampling: at the display size, and the anti-aliasing reads the stage's buffer
        app.SetTemporalUpscale(WO, HO);
        app.SetAntiAliasing(true);
        if (app.SharpenedBackBuffer()->Bytes() != (size_t)WO * HO * 4) { std::fprintf(stderr, "the stage's buffer has not the display's size\n"); return 8; }
        d.frame();
        d.frame();
        d.grab(app.TemporalUpscaleBackBuffer(), "sharp_up_in.bin");
        d.grab(app.SharpenedBackBuffer(), "sharp_up.bin");
        d.grab(app.AntiAliasedBackBuffer(), "sharp_up_aa.bin");
        app.SetAntiAliasing(false);
        app.SetTemporalUpscale(0, 0);
        if (app.SharpenedBackBuffer()->Bytes() != (size_t)d.W * H * 4) { std::fprintf(stderr, "the stage's buffer did not return to the frame's size\n"); return 9; }

        // off again
        app.SetSharpening(false);
        if (app.Sharpening() || app.SharpenedBackBuffer()) { std::fprintf(stderr, "SetSharpening(false)\n"); return 10; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("sharpen driver ok %ux%u\n", d.W, H);
        return 0;
    }, 10);
}
