// spot_driver.cpp -- the C++ veneer's local lights: CRYCHIC::SetLocalLights with point and spot lists read from raw files, then
// Update / Draw as a reference call site would; the frame goes back for comparison with the Python path
// (tests/test_spot_lights.py).  Usage: spot_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
// <dir> holds the planes veneer_driver reads plus points.bin and spots.bin (arrays of Light).
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
static void put(ID3D12Resource* r, const std::string& path, hipStream_t s)
{
    auto b = slurp(path);
    if (b.size() != r->Bytes()) { std::fprintf(stderr, "%s: %zu bytes, resource has %zu\n", path.c_str(), b.size(), r->Bytes()); std::exit(2); }
    r->Upload(b.data(), b.size(), s);
    CrychicHipThrowIfFailed(hipStreamSynchronize(s));
}
static std::vector<Light> lights(const std::string& path)
{
    auto b = slurp(path);
    std::vector<Light> v(b.size() / sizeof(Light));
    std::memcpy(v.data(), b.data(), v.size() * sizeof(Light));
    return v;
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
        app.mRunProducerPasses = false;
        if (!app.Initialize()) return 3;
        hipStream_t s = app.CommandList()->Stream();
        put(app.DepthStencilBuffer(), dir + "/depth.bin", s);
        put(app.mSsao->NormalMap(), dir + "/normal.bin", s);
        for (int i = 0; i < 3; ++i) put(app.mDeferred->Resource(i), dir + "/g" + std::to_string(i) + ".bin", s);
        for (int i = 0; i < 4; ++i) put(app.mShadowMap->Resource(i), dir + "/shadow" + std::to_string(i) + ".bin", s);
        auto cube = std::make_unique<ID3D12Resource>((size_t)6 * CD * CD * 4, ID3D12Resource::DEFAULT_HEAP);
        put(cube.get(), dir + "/cube.bin", s);
        app.SetCubeMap(std::move(cube), CD);

        const std::vector<Light> points = lights(dir + "/points.bin"), spots = lights(dir + "/spots.bin");
        // errors throw CrychicException, as everywhere in the veneer
        bool threw = false;
        try { app.SetLocalLights(nullptr, 1, nullptr, 0); } catch (const CrychicException& e) { threw = e.Status == CRYCHIC_E_INVALID_ARG; }
        if (!threw) { std::fprintf(stderr, "SetLocalLights(nullptr, 1) did not throw\n"); return 4; }
        threw = false;
        std::vector<Light> many(1025);
        try { app.SetLocalLights(nullptr, 0, many.data(), 1025); } catch (const CrychicException& e) { threw = e.Status == CRYCHIC_E_INVALID_ARG; }
        if (!threw) { std::fprintf(stderr, "SetLocalLights(1025 spots) did not throw\n"); return 4; }

        GameTimer gt;
        auto frame = [&](const std::string& name) {
            for (int f = 0; f < 4; ++f) {               // cycles the frame-resource ring
                gt.Tick(1.0f / 60.0f);
                app.Update(gt);
                app.Draw(gt);
            }
            app.CommandList()->Flush();
            std::vector<uint8_t> out((size_t)W * H * 4);
            app.CurrentBackBuffer()->Download(out.data(), out.size(), s);
            app.CommandList()->Flush();
            dump(dir + "/" + name, out.data(), out.size());
        };
        app.SetLocalLights(points.data(), (uint32_t)points.size(), spots.data(), (uint32_t)spots.size());
        frame("out.bin");
        app.SetLocalLights(nullptr, 0, nullptr, 0);     // today's behaviour again
        frame("out_nolights.bin");
        dump(dir + "/pass_cb.bin", &app.mCurrFrameResource->PassCB->Element(0), sizeof(PassConstants));
        dump(dir + "/ssao_cb.bin", &app.mCurrFrameResource->SsaoCB->Element(0), sizeof(SsaoConstants));
        std::printf("spot driver ok %ux%u\n", W, H);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
