// fog_driver.cpp -- CRYCHIC::SetFog through the C++ veneer (include/crychic/CRYCHIC.h): the application's built-in scene is drawn with the
// switch off (plain.bin = the back buffer; depth.bin, shadow0..3.bin and pass_cb.bin = what the pass reads of the frame), then on
// (fog.bin), with parameters of the caller's (fog_params.bin), together with SetAntiAliasing (fog_frame.bin = the back buffer,
// fog_aa.bin = the second back buffer), then off again (plain_again.bin); a parameter outside its range must be refused, and a strip
// with the switch on must make Draw throw (tests/test_fog_veneer.py).
// Usage: fog_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [](PostDriver& d) {
        CRYCHIC& app = d.app;
        const std::string& dir = d.dir;
        const UINT W = d.W, H = d.H;
        if (app.Fog()) { std::fprintf(stderr, "fog is on by default\n"); return 4; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");
        d.grab(app.DepthStencilBuffer(), "depth.bin");
        for (int i = 0; i < 4; ++i) d.grab(app.mShadowMap->Resource(i), "shadow" + std::to_string(i) + ".bin");
        dump(dir + "/pass_cb.bin", &app.mMainPassCB, sizeof app.mMainPassCB);

        // a parameter outside its range is refused and leaves the switch as it was
        int refused = 0;
        crychic_fog_params bad;
        crychic_fog_default_params(&bad);
        bad.steps = CRYCHIC_FOG_MAX_STEPS + 1;
        try { app.SetFog(true, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 1 || app.Fog()) { std::fprintf(stderr, "a bad parameter was not refused\n"); return 5; }

        app.SetFog(true);
        if (!app.Fog()) { std::fprintf(stderr, "SetFog(true)\n"); return 6; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "fog.bin");

        // a strip with the switch on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        d.gt.Tick(1.0f / 60.0f);
        app.Update(d.gt);
        try { app.Draw(d.gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 2) { std::fprintf(stderr, "a strip with fog on did not throw\n"); return 7; }
        app.SetWholeFrame();

        // the caller's parameters reach the pass
        crychic_fog_params p;
        crychic_fog_default_params(&p);
        p.density = 0.08f; p.steps = 7; p.sun[0] = 250; p.sun[1] = 200; p.sun[2] = 90;
        app.SetFog(true, &p);
        d.frame();
        d.grab(app.CurrentBackBuffer(), "fog_params.bin");

        // with the anti-aliasing: lighting, fog in place, then the anti-aliasing of the fogged frame into the second back buffer
        app.SetFog(true);
        app.SetAntiAliasing(true);
        d.frame();
        d.grab(app.CurrentBackBuffer(), "fog_frame.bin");
        d.grab(app.AntiAliasedBackBuffer(), "fog_aa.bin");
        app.SetAntiAliasing(false);

        // off again
        app.SetFog(false);
        if (app.Fog()) { std::fprintf(stderr, "SetFog(false)\n"); return 9; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("fog driver ok %ux%u\n", W, H);
        return 0;
    });
}
