// ssr_driver.cpp -- CRYCHIC::SetScreenSpaceReflections through the C++ veneer (include/crychic/CRYCHIC.h): the application's built-in
// scene is drawn with the switch off (plain.bin = the back buffer; depth.bin, g0..2.bin, shadow0..3.bin and pass_cb.bin = what the
// passes read of the frame), then on (ssr.bin = the pass's buffer, ssr_back.bin = the back buffer, present_ssr.ppm = what Present
// writes), with parameters of the caller's (ssr_params.bin), in front of the fog (ssr_fog.bin, ssr_fog_back.bin), in front of the depth
// of field (ssr_dof_front.bin = the pass's buffer, ssr_dof.bin = the depth of field's, present_dof.ppm), then off again
// (plain_again.bin); a parameter outside its range must be refused, and a strip with the switch on must make Draw throw
// (tests/test_ssr_veneer.py).
// Usage: ssr_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [](PostDriver& d) {
        CRYCHIC& app = d.app;
        const std::string& dir = d.dir;
        const UINT W = d.W, H = d.H;
        if (app.ScreenSpaceReflections()) { std::fprintf(stderr, "screen-space reflections are on by default\n"); return 4; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");
        d.grab(app.DepthStencilBuffer(), "depth.bin");
        for (int i = 0; i < 3; ++i) d.grab(app.mDeferred->Resource(i), "g" + std::to_string(i) + ".bin");
        for (int i = 0; i < 4; ++i) d.grab(app.mShadowMap->Resource(i), "shadow" + std::to_string(i) + ".bin");
        dump(dir + "/pass_cb.bin", &app.mMainPassCB, sizeof app.mMainPassCB);

        // a parameter outside its range is refused and leaves the switch as it was
        int refused = 0;
        crychic_ssr_params bad;
        crychic_ssr_default_params(&bad);
        bad.steps = CRYCHIC_SSR_MAX_STEPS + 1;
        try { app.SetScreenSpaceReflections(true, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 1 || app.ScreenSpaceReflections() || app.ScreenSpaceReflectionsBackBuffer()) { std::fprintf(stderr, "a bad parameter was not refused\n"); return 5; }

        app.SetScreenSpaceReflections(true);
        if (!app.ScreenSpaceReflections()) { std::fprintf(stderr, "SetScreenSpaceReflections(true)\n"); return 6; }
        d.frame();
        d.grab(app.ScreenSpaceReflectionsBackBuffer(), "ssr.bin");
        d.grab(app.CurrentBackBuffer(), "ssr_back.bin");
        app.Present(dir + "/present_ssr.ppm");

        // a strip with the switch on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        d.gt.Tick(1.0f / 60.0f);
        app.Update(d.gt);
        try { app.Draw(d.gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 2) { std::fprintf(stderr, "a strip with screen-space reflections on did not throw\n"); return 7; }
        app.SetWholeFrame();

        // the caller's parameters reach the pass
        crychic_ssr_params p;
        crychic_ssr_default_params(&p);
        p.maxDistance = 12.0f; p.thickness = 1.5f; p.maxRoughness = 1.0f; p.steps = 48; p.edgeFade = 8; p.intensity = 200;
        app.SetScreenSpaceReflections(true, &p);
        d.frame();
        d.grab(app.ScreenSpaceReflectionsBackBuffer(), "ssr_params.bin");

        // in front of the fog: the fog works in place on the pass's buffer, the back buffer stays the plain frame
        app.SetScreenSpaceReflections(true);
        app.SetFog(true);
        d.frame();
        d.grab(app.ScreenSpaceReflectionsBackBuffer(), "ssr_fog.bin");
        d.grab(app.CurrentBackBuffer(), "ssr_fog_back.bin");
        app.SetFog(false);

        // in front of the depth of field
        app.SetDepthOfField(true);
        d.frame();
        d.grab(app.ScreenSpaceReflectionsBackBuffer(), "ssr_dof_front.bin");
        d.grab(app.DepthOfFieldBackBuffer(), "ssr_dof.bin");
        app.Present(dir + "/present_dof.ppm");
        app.SetDepthOfField(false);

        // off again
        app.SetScreenSpaceReflections(false);
        if (app.ScreenSpaceReflections() || app.ScreenSpaceReflectionsBackBuffer()) { std::fprintf(stderr, "SetScreenSpaceReflections(false)\n"); return 9; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("ssr driver ok %ux%u\n", W, H);
        return 0;
    });
}
