// bloom_driver.cpp -- CRYCHIC::SetBloom through the C++ veneer (include/crychic/CRYCHIC.h): the application's built-in scene is drawn
// with the switch off (plain.bin = the back buffer), then on with parameters of the caller's (bloom_frame.bin = the back buffer, bloom.bin =
// the pass's buffer), with the defaults (bloom_default.bin), together with SetDepthOfField and SetAntiAliasing (bloom_dof_in.bin = the
// depth-of-field buffer the pass read, bloom_dof.bin = the pass's buffer, bloom_dof_aa.bin = the anti-aliased buffer), then off again
// (plain_again.bin); parameters outside their ranges must be refused, and a strip with the switch on must make Draw throw
// (tests/test_bloom_veneer.py).
// Usage: bloom_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
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
        if (app.Bloom() || app.BloomBackBuffer()) { std::fprintf(stderr, "bloom is on by default\n"); return 4; }
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
        frame();
        grab(app.CurrentBackBuffer(), "bloom_frame.bin");
        grab(app.BloomBackBuffer(), "bloom.bin");

        // a strip with the switch on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        gt.Tick(1.0f / 60.0f);
        app.Update(gt);
        try { app.Draw(gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 8) { std::fprintf(stderr, "a strip with bloom on did not throw\n"); return 7; }
        app.SetWholeFrame();

        // the defaults
        app.SetBloom(true);
        frame();
        grab(app.BloomBackBuffer(), "bloom_default.bin");

        // behind the depth of field and in front of the anti-aliasing
        app.SetBloom(true, &low);
        app.SetDepthOfField(true);
        app.SetAntiAliasing(true);
        frame();
        grab(app.DepthOfFieldBackBuffer(), "bloom_dof_in.bin");
        grab(app.BloomBackBuffer(), "bloom_dof.bin");
        grab(app.AntiAliasedBackBuffer(), "bloom_dof_aa.bin");
        app.SetAntiAliasing(false);
        app.SetDepthOfField(false);

        // off again
        app.SetBloom(false);
        if (app.Bloom() || app.BloomBackBuffer()) { std::fprintf(stderr, "SetBloom(false)\n"); return 9; }
        frame();
        grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("bloom driver ok %ux%u\n", W, H);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
