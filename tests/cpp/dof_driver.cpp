// dof_driver.cpp -- CRYCHIC::SetDepthOfField through the C++ veneer (include/crychic/CRYCHIC.h): the application's built-in scene is
// drawn with the switch off (plain.bin = the back buffer; depth.bin and pass_cb.bin = what the pass reads of the frame), then on
// (dof_frame.bin = the back buffer, dof.bin = the pass's buffer), with parameters of the caller's (dof_params.bin), together with
// SetAntiAliasing (dof_aa.bin = the anti-aliased buffer), then off again (plain_again.bin); a parameter outside its range must be
// refused, and a strip with the switch on must make Draw throw (tests/test_dof_veneer.py).
// Usage: dof_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [](PostDriver& d) {
        CRYCHIC& app = d.app;
        const std::string& dir = d.dir;
        const UINT W = d.W, H = d.H;
        if (app.DepthOfField() || app.DepthOfFieldBackBuffer()) { std::fprintf(stderr, "depth of field is on by default\n"); return 4; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");
        d.grab(app.DepthStencilBuffer(), "depth.bin");
        dump(dir + "/pass_cb.bin", &app.mMainPassCB, sizeof app.mMainPassCB);

        // a parameter outside its range is refused and leaves the switch as it was
        int refused = 0;
        crychic_dof_params bad;
        crychic_dof_default_params(&bad);
        bad.maxRadius = CRYCHIC_DOF_MAX_RADIUS + 1;
        try { app.SetDepthOfField(true, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 1 || app.DepthOfField()) { std::fprintf(stderr, "a bad parameter was not refused\n"); return 5; }

        app.SetDepthOfField(true);
        if (!app.DepthOfField() || !app.DepthOfFieldBackBuffer()) { std::fprintf(stderr, "SetDepthOfField(true)\n"); return 6; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "dof_frame.bin");
        d.grab(app.DepthOfFieldBackBuffer(), "dof.bin");

        // a strip with the switch on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        d.gt.Tick(1.0f / 60.0f);
        app.Update(d.gt);
        try { app.Draw(d.gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 2) { std::fprintf(stderr, "a strip with depth of field on did not throw\n"); return 7; }
        app.SetWholeFrame();

        // the caller's parameters reach the pass
        crychic_dof_params p;
        crychic_dof_default_params(&p);
        p.focusDistance = 30.0f; p.aperture = 20.0f; p.maxRadius = 5;
        app.SetDepthOfField(true, &p);
        d.frame();
        d.grab(app.DepthOfFieldBackBuffer(), "dof_params.bin");

        // with the anti-aliasing: lighting, the lens blur into its buffer, then the anti-aliasing of that buffer
        app.SetDepthOfField(true);
        app.SetAntiAliasing(true);
        d.frame();
        d.grab(app.AntiAliasedBackBuffer(), "dof_aa.bin");
        app.SetAntiAliasing(false);

        // off again
        app.SetDepthOfField(false);
        if (app.DepthOfField() || app.DepthOfFieldBackBuffer()) { std::fprintf(stderr, "SetDepthOfField(false)\n"); return 9; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("dof driver ok %ux%u\n", W, H);
        return 0;
    });
}
