// post_aa_driver.cpp -- CRYCHIC::SetAntiAliasing through the C++ veneer (include/crychic/CRYCHIC.h), as a reference call site would
// use the framework's Set4xMsaaState: the application's built-in scene is drawn with the switch off (plain.bin = the back buffer,
// plain.ppm = what Present writes), then on (frame.bin = the back buffer under the pass, aa.bin = the second back buffer, aa.ppm =
// what Present writes), resized there and back and drawn again (resized_aa.bin), then off again (plain_again.*); a strip with the switch on must make Draw throw
// (tests/test_post_aa_veneer.py).
// Usage: post_aa_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
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
        if (app.AntiAliasing() || app.AntiAliasedBackBuffer()) { std::fprintf(stderr, "anti-aliasing is on by default\n"); return 4; }
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
        frame();
        grab(app.CurrentBackBuffer(), "frame.bin");
        grab(app.AntiAliasedBackBuffer(), "aa.bin");
        app.Present(dir + "/aa.ppm");

        // a strip with the switch on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        gt.Tick(1.0f / 60.0f);
        app.Update(gt);
        try { app.Draw(gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 2) { std::fprintf(stderr, "a strip with anti-aliasing on did not throw\n"); return 7; }
        app.SetWholeFrame();

        // OnResize re-creates the second back buffer with the first; back at the first size the frame is the same again
        app.Resize(W + 2, H - 2);
        if (app.AntiAliasedBackBuffer()->Bytes() != (size_t)(W + 2) * (H - 2) * 4) { std::fprintf(stderr, "the second back buffer was not resized\n"); return 8; }
        app.Resize(W, H);
        frame();
        grab(app.AntiAliasedBackBuffer(), "resized_aa.bin");

        // off again: the second buffer goes, Present writes the plain frame
        app.SetAntiAliasing(false);
        if (app.AntiAliasing() || app.AntiAliasedBackBuffer()) { std::fprintf(stderr, "SetAntiAliasing(false)\n"); return 9; }
        frame();
        grab(app.CurrentBackBuffer(), "plain_again.bin");
        app.Present(dir + "/plain_again.ppm");
        std::printf("post aa driver ok %ux%u\n", W, H);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
