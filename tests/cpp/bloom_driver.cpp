// bloom_driver.cpp -- CRYCHIC::SetBloom through the C++ veneer (include/crychic/CRYCHIC.h): the application's built-in scene is drawn
// with the switch off (plain.bin = the back buffer), then on with parameters of the caller's (bloom_frame.bin = the back buffer, bloom.bin =
// the pass's buffer), with the defaults (bloom_default.bin), together with SetDepthOfField and SetAntiAliasing (bloom_dof_in.bin = the
// depth-of-field buffer the pass read, bloom_dof.bin = the pass's buffer, bloom_dof_aa.bin = the anti-aliased buffer), then off again
// (plain_again.bin); parameters outside their ranges must be refused, and a strip with the switch on must make Draw throw
// (tests/test_bloom_veneer.py).
// Usage: bloom_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [](PostDriver& d) {
        CRYCHIC& app = d.app;
        const UINT W = d.W, H = d.H;
        if (app.Bloom() || app.BloomBackBuffer()) { std::fprintf(stderr, "bloom is on by default\n"); return 4; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");

        // parameters outside their ranges are refused and leave the switch as it was
        int refused = 0;
        for (int which = 0; which < 7; ++which) {
            crychic_bloom_params bad;
            crychic_bloom_default_params(&bad);
            if (which == 0) bad.threshold = 256;
            if (which == 1) bad.knee = 0;
            if (which == 2) bad.knee = 256;
            if (which == 3) bad.scatter = 257;
            if (which == 4) bad.intensity = 1025;
            if (which == 5) bad.levels = CRYCHIC_BLOOM_MAX_LEVELS + 1;
            if (which == 6) bad.reserved[1] = 1;
            try { app.SetBloom(true, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        }
        if (refused != 7 || app.Bloom() || app.BloomBackBuffer()) { std::fprintf(stderr, "a bad parameter was not refused\n"); return 5; }

        // a caller's parameters reach the pass (tests/test_bloom_veneer.py states the same values)
        crychic_bloom_params low;
        crychic_bloom_default_params(&low);
        low.threshold = 160; low.intensity = 64;
        app.SetBloom(true, &low);
        if (!app.Bloom() || !app.BloomBackBuffer()) { std::fprintf(stderr, "SetBloom(true)\n"); return 6; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "bloom_frame.bin");
        d.grab(app.BloomBackBuffer(), "bloom.bin");

        // a strip with the switch on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        d.gt.Tick(1.0f / 60.0f);
        app.Update(d.gt);
        try { app.Draw(d.gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 8) { std::fprintf(stderr, "a strip with bloom on did not throw\n"); return 7; }
        app.SetWholeFrame();

        // the defaults
        app.SetBloom(true);
        d.frame();
        d.grab(app.BloomBackBuffer(), "bloom_default.bin");

        // behind the depth of field and in front of the anti-aliasing
        app.SetBloom(true, &low);
        app.SetDepthOfField(true);
        app.SetAntiAliasing(true);
        d.frame();
        d.grab(app.DepthOfFieldBackBuffer(), "bloom_dof_in.bin");
        d.grab(app.BloomBackBuffer(), "bloom_dof.bin");
        d.grab(app.AntiAliasedBackBuffer(), "bloom_dof_aa.bin");
        app.SetAntiAliasing(false);
        app.SetDepthOfField(false);

        // off again
        app.SetBloom(false);
        if (app.Bloom() || app.BloomBackBuffer()) { std::fprintf(stderr, "SetBloom(false)\n"); return 9; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("bloom driver ok %ux%u\n", W, H);
        return 0;
    });
}
