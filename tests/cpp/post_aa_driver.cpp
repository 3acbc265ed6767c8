// post_aa_driver.cpp -- CRYCHIC::SetAntiAliasing through the C++ veneer (include/crychic/CRYCHIC.h), as a reference call site would
// use the framework's Set4xMsaaState: the application's built-in scene is drawn with the switch off (plain.bin = the back buffer,
// plain.ppm = what Present writes), then on (frame.bin = the back buffer under the pass, aa.bin = the second back buffer, aa.ppm =
// what Present writes), resized there and back and drawn again (resized_aa.bin), then off again (plain_again.*); a strip with the switch on must make Draw throw
// (tests/test_post_aa_veneer.py).
// Usage: post_aa_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [](PostDriver& d) {
        CRYCHIC& app = d.app;
        const std::string& dir = d.dir;
        const UINT W = d.W, H = d.H;
        if (app.AntiAliasing() || app.AntiAliasedBackBuffer()) { std::fprintf(stderr, "anti-aliasing is on by default\n"); return 4; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");
        app.Present(dir + "/plain.ppm");

        // a parameter outside its range is refused and leaves the switch as it was
        int refused = 0;
        crychic_aa_params bad;
        crychic_aa_default_params(&bad);
        bad.searchSteps = CRYCHIC_AA_MAX_SEARCH + 1;
        try { app.SetAntiAliasing(true, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 1 || app.AntiAliasing()) { std::fprintf(stderr, "a bad parameter was not refused\n"); return 5; }

        app.SetAntiAliasing(true);
        if (!app.AntiAliasing() || !app.AntiAliasedBackBuffer()) { std::fprintf(stderr, "SetAntiAliasing(true)\n"); return 6; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "frame.bin");
        d.grab(app.AntiAliasedBackBuffer(), "aa.bin");
        app.Present(dir + "/aa.ppm");

        // a strip with the switch on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        d.gt.Tick(1.0f / 60.0f);
        app.Update(d.gt);
        try { app.Draw(d.gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 2) { std::fprintf(stderr, "a strip with anti-aliasing on did not throw\n"); return 7; }
        app.SetWholeFrame();

        // OnResize re-creates the second back buffer with the first; back at the first size the frame is the same again
        app.Resize(W + 2, H - 2);
        if (app.AntiAliasedBackBuffer()->Bytes() != (size_t)(W + 2) * (H - 2) * 4) { std::fprintf(stderr, "the second back buffer was not resized\n"); return 8; }
        app.Resize(W, H);
        d.frame();
        d.grab(app.AntiAliasedBackBuffer(), "resized_aa.bin");

        // off again: the second buffer goes, Present writes the plain frame
        app.SetAntiAliasing(false);
        if (app.AntiAliasing() || app.AntiAliasedBackBuffer()) { std::fprintf(stderr, "SetAntiAliasing(false)\n"); return 9; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");
        app.Present(dir + "/plain_again.ppm");
        std::printf("post aa driver ok %ux%u\n", W, H);
        return 0;
    });
}
