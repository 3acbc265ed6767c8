// sky_driver.cpp -- CRYCHIC::RenderSky and CRYCHIC::SetProceduralSky through the C++ veneer (include/crychic/CRYCHIC.h): the
// application's built-in scene is drawn with neither (plain.bin = the back buffer), then after an explicit RenderSky with parameters
// of the caller's (sky_cube.bin = the bound cube map, sky.bin = the back buffer), then with SetProceduralSky(true) over two frames
// between which the lights turn by SetLightRotationAngle (follow_cube0/1.bin, follow_cb0/1.bin = the pass constants,
// follow0/1.bin = the back buffers), over a third frame whose light stands still (no further sky launch), and with the switch off again (off.bin, the cube map staying
// bound); a parameter outside its range must be refused (tests/test_sky_veneer.py).
// Usage: sky_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [](PostDriver& d) {
        CRYCHIC& app = d.app;
        const std::string& dir = d.dir;
        if (app.ProceduralSky() || app.SkyRenders() != 0) { std::fprintf(stderr, "the procedural sky is on by default\n"); return 4; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");
        if (app.SkyRenders() != 0) { std::fprintf(stderr, "a plain frame rendered a sky\n"); return 4; }

        int refused = 0;
        crychic_sky_params bad;
        crychic_sky_default_params(&bad);
        bad.viewSteps = CRYCHIC_SKY_MAX_VIEW_STEPS + 1;
        try { app.SetProceduralSky(true, &bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        try { app.RenderSky(&bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        try { app.RenderSky(nullptr, 1); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 3 || app.ProceduralSky() || app.SkyRenders() != 0) { std::fprintf(stderr, "a bad parameter was not refused\n"); return 5; }

        // explicit: the caller's parameters, the bound size, one level
        crychic_sky_params p;
        crychic_sky_default_params(&p);
        p.sunDir[0] = 0.3f; p.sunDir[1] = 0.2f; p.sunDir[2] = -0.8f; p.altitude = 1.5f; p.viewSteps = 9; p.sunSteps = 5;
        app.RenderSky(&p, 0, 1);
        if (app.SkyRenders() != 1 || app.CubeMapLevels() != 1) { std::fprintf(stderr, "RenderSky\n"); return 6; }
        d.grab(app.CubeMap(), "sky_cube.bin");
        d.frame();
        d.grab(app.CurrentBackBuffer(), "sky.bin");

        // following the sun: the application turns its lights between the two frames (the reference's own rate of turning is zero)
        app.SetProceduralSky(true);
        for (int k = 0; k < 2; ++k) {
            app.SetLightRotationAngle(0.5f * k);
            d.frame();
            if (app.SkyRenders() != (UINT)(2 + k)) { std::fprintf(stderr, "frame %d under SetProceduralSky rendered no sky\n", k); return 7; }
            d.grab(app.CubeMap(), "follow_cube" + std::to_string(k) + ".bin");
            dump(dir + "/follow_cb" + std::to_string(k) + ".bin", &app.mMainPassCB, sizeof app.mMainPassCB);
            d.grab(app.CurrentBackBuffer(), "follow" + std::to_string(k) + ".bin");
        }
        // the light stands still (no Update): no sky launch
        app.Draw(d.gt);
        app.CommandList()->Flush();
        if (app.SkyRenders() != 3) { std::fprintf(stderr, "a frame under an unchanged light rendered a sky\n"); return 8; }
        d.grab(app.CurrentBackBuffer(), "follow_still.bin");

        app.SetProceduralSky(false);
        d.frame();
        if (app.ProceduralSky() || app.SkyRenders() != 3) { std::fprintf(stderr, "SetProceduralSky(false)\n"); return 9; }
        d.grab(app.CubeMap(), "off_cube.bin");
        std::printf("sky driver ok %ux%u\n", d.W, d.H);
        return 0;
    });
}
