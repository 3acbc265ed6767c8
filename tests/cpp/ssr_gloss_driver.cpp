// ssr_gloss_driver.cpp -- CRYCHIC::SetScreenSpaceReflectionGloss through the C++ veneer (include/crychic/CRYCHIC.h): the application's
// built-in scene is drawn with the switches off (plain.bin = the back buffer; depth.bin, g0..2.bin, shadow0..3.bin and pass_cb.bin =
// what the passes read of the frame), with the reflections alone (ssr.bin), with the gloss over them at the default parameters
// (gloss_default.bin) and at the caller's (gloss.bin = the pass's buffer, gloss_back.bin = the back buffer, pyramid.bin = the first
// crychic_ssr_pyramid_bytes bytes of the pyramid, present_gloss.ppm = what Present writes), in front of the fog (gloss_fog.bin), after
// a resize and back (gloss_resized.bin), with the gloss off again (ssr_again.bin) and with both off (plain_again.bin).  A parameter
// outside its range must be refused, and the gloss without the reflections must make Draw throw (tests/test_ssr_gloss_veneer.py).
// Usage: ssr_gloss_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [](PostDriver& d) {
        CRYCHIC& app = d.app;
        const std::string& dir = d.dir;
        const UINT W = d.W, H = d.H;
        if (app.ScreenSpaceReflectionGloss() || app.ScreenSpaceReflectionPyramid()) { std::fprintf(stderr, "the gloss is on by default\n"); return 4; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");
        d.grab(app.DepthStencilBuffer(), "depth.bin");
        for (int i = 0; i < 3; ++i) d.grab(app.mDeferred->Resource(i), "g" + std::to_string(i) + ".bin");
        for (int i = 0; i < 4; ++i) d.grab(app.mShadowMap->Resource(i), "shadow" + std::to_string(i) + ".bin");
        dump(dir + "/pass_cb.bin", &app.mMainPassCB, sizeof app.mMainPassCB);

        // a parameter outside its range is refused and leaves the switch as it was
        int refused = 0;
        crychic_ssr_gloss_params bad;
        crychic_ssr_gloss_default_params(&bad);
        bad.levels = CRYCHIC_SSR_GLOSS_MAX_LEVELS + 1;
        try { app.SetScreenSpaceReflectionGloss(true, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        bad.levels = 6; bad.coneScale = 17.0f;
        try { app.SetScreenSpaceReflectionGloss(true, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 2 || app.ScreenSpaceReflectionGloss() || app.ScreenSpaceReflectionPyramid()) { std::fprintf(stderr, "a bad parameter was not refused\n"); return 5; }

        // the gloss without the reflections: Draw throws before it issues anything, and works again afterwards
        app.SetScreenSpaceReflectionGloss(true);
        d.gt.Tick(1.0f / 60.0f);
        app.Update(d.gt);
        try { app.Draw(d.gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 3) { std::fprintf(stderr, "the gloss without the reflections did not throw\n"); return 6; }
        app.SetScreenSpaceReflectionGloss(false);

        app.SetScreenSpaceReflections(true);
        d.frame();
        d.grab(app.ScreenSpaceReflectionsBackBuffer(), "ssr.bin");

        app.SetScreenSpaceReflectionGloss(true);                // the defaults
        if (!app.ScreenSpaceReflectionGloss() || !app.ScreenSpaceReflectionPyramid()) { std::fprintf(stderr, "SetScreenSpaceReflectionGloss(true)\n"); return 7; }
        d.frame();
        d.grab(app.ScreenSpaceReflectionsBackBuffer(), "gloss_default.bin");

        crychic_ssr_gloss_params g;
        crychic_ssr_gloss_default_params(&g);
        g.coneScale = 1.0f; g.levels = 5;
        app.SetScreenSpaceReflectionGloss(true, &g);
        d.frame();
        d.grab(app.ScreenSpaceReflectionsBackBuffer(), "gloss.bin");
        d.grab(app.CurrentBackBuffer(), "gloss_back.bin");
        {
            const size_t n = crychic_ssr_pyramid_bytes(W, H, g.levels);
            std::vector<uint8_t> host(n);
            CrychicHipThrowIfFailed(hipMemcpy(host.data(), app.ScreenSpaceReflectionPyramid()->Data(), n, hipMemcpyDeviceToHost));
            dump(dir + "/pyramid.bin", host.data(), n);
        }
        app.Present(dir + "/present_gloss.ppm");

        // in front of the fog: the fog works in place on the pass's buffer
        app.SetFog(true);
        d.frame();
        d.grab(app.ScreenSpaceReflectionsBackBuffer(), "gloss_fog.bin");
        app.SetFog(false);

        // OnResize re-creates the pyramid: another size and back
        app.Resize(W + 2, H - 2);
        if (app.ScreenSpaceReflectionPyramid()->Bytes() != crychic_ssr_pyramid_bytes(W + 2, H - 2, CRYCHIC_SSR_GLOSS_MAX_LEVELS)) {
            std::fprintf(stderr, "the pyramid was not resized\n");
            return 9;
        }
        app.Resize(W, H);
        d.frame();
        d.grab(app.ScreenSpaceReflectionsBackBuffer(), "gloss_resized.bin");

        app.SetScreenSpaceReflectionGloss(false);
        if (app.ScreenSpaceReflectionGloss() || app.ScreenSpaceReflectionPyramid()) { std::fprintf(stderr, "SetScreenSpaceReflectionGloss(false)\n"); return 8; }
        d.frame();
        d.grab(app.ScreenSpaceReflectionsBackBuffer(), "ssr_again.bin");
        app.SetScreenSpaceReflections(false);
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("ssr gloss driver ok %ux%u\n", W, H);
        return 0;
    });
}
