// dof_driver.cpp -- CRYCHIC::SetDepthOfField through the C++ veneer (include/crychic/CRYCHIC.h): the application's built-in scene is
// drawn with the switch off (plain.bin = the back buffer; depth.bin and pass_cb.bin = what the pass reads of the frame), then on
// (dof_frame.bin = the back buffer, dof.bin = the pass's buffer), with parameters of the caller's (dof_params.bin), together with
// SetAntiAliasing (dof_aa.bin = the anti-aliased buffer), then off again (plain_again.bin); a parameter outside its range must be
// refused, and a strip with the switch on must make Draw throw (tests/test_dof_veneer.py).
// Usage: dof_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "crychic/CRYCHIC.h"

static std::vector<char> slurp(const std::string& p)
{
    std::ifstream f(p, std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", p.c_str()); std::exit(2); }
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static void dump(const std::string& p, const void* d, size_t n)
{
    std::ofstream f(p, std::ios::binary);
    f.write(static_cast<const char*>(d), (std::streamsize)n);
}

int main(int argc, char** argv)
{
    if (argc < 8) { std::fprintf(stderr, "usage\n"); return 2; }
    const std::string dir = argv[1];
    const UINT W = std::atoi(argv[2]), H = std::atoi(argv[3]), SD = std::atoi(argv[4]), CD = std::atoi(argv[5]);
    try {
        CRYCHIC app(0, W, H);
        app.mShadowMapSize = SD;
        app.mBlurCount = std::atoi(argv[6]);
        app.mNumDirLights = std::atoi(argv[7]);
        app.mSkyEnabled = true;
        app.mRunProducerPasses = true;
        if (!app.Initialize()) return 3;
        hipStream_t s = app.CommandList()->Stream();
        if (app.DepthOfField() || app.DepthOfFieldBackBuffer()) { std::fprintf(stderr, "depth of field is on by default\n"); return 4; }
        auto cubeBytes = slurp(dir + "/cube.bin");
        auto cube = std::make_unique<ID3D12Resource>((size_t)6 * CD * CD * 4, ID3D12Resource::DEFAULT_HEAP);
        if (cubeBytes.size() != cube->Bytes()) { std::fprintf(stderr, "cube.bin size\n"); return 2; }
        cube->Upload(cubeBytes.data(), cubeBytes.size(), s);
        CrychicHipThrowIfFailed(hipStreamSynchronize(s));
        app.SetCubeMap(std::move(cube), CD);

        GameTimer gt;
        auto frame = [&] { gt.Tick(1.0f / 60.0f); app.Update(gt); app.Draw(gt); app.CommandList()->Flush(); };
        auto grab = [&](ID3D12Resource* r, const std::string& name) {
            std::vector<char> h(r->Bytes());
            r->Download(h.data(), h.size(), s);
            app.CommandList()->Flush();
            dump(dir + "/" + name, h.data(), h.size());
        };
        frame();
        grab(app.CurrentBackBuffer(), "plain.bin");
        grab(app.DepthStencilBuffer(), "depth.bin");
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
        frame();
        grab(app.CurrentBackBuffer(), "dof_frame.bin");
        grab(app.DepthOfFieldBackBuffer(), "dof.bin");

        // a strip with the switch on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        gt.Tick(1.0f / 60.0f);
        app.Update(gt);
        try { app.Draw(gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 2) { std::fprintf(stderr, "a strip with depth of field on did not throw\n"); return 7; }
        app.SetWholeFrame();

        // the caller's parameters reach the pass
        crychic_dof_params p;
        crychic_dof_default_params(&p);
        p.focusDistance = 30.0f; p.aperture = 20.0f; p.maxRadius = 5;
        app.SetDepthOfField(true, &p);
        frame();
        grab(app.DepthOfFieldBackBuffer(), "dof_params.bin");

        // with the anti-aliasing: lighting, the lens blur into its buffer, then the anti-aliasing of that buffer
        app.SetDepthOfField(true);
        app.SetAntiAliasing(true);
        frame();
        grab(app.AntiAliasedBackBuffer(), "dof_aa.bin");
        app.SetAntiAliasing(false);

        // off again
        app.SetDepthOfField(false);
        if (app.DepthOfField() || app.DepthOfFieldBackBuffer()) { std::fprintf(stderr, "SetDepthOfField(false)\n"); return 9; }
        frame();
        grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("dof driver ok %ux%u\n", W, H);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
