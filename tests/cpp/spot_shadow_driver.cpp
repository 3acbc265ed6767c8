// spot_shadow_driver.cpp -- the C++ veneer's shadowed spot lights: CRYCHIC::SetLocalLights + SetSpotShadows, then Update / Draw as a
// reference call site would; frames go back for comparison with the Python path (tests/test_spot_shadows_veneer.py).
// Usage: spot_shadow_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights> <count> <dim>
// <dir> holds the planes veneer_driver reads, spots.bin (an array of Light), spotmap<k>.bin (the first <count> maps, dim x dim D24)
// and scene_spots.bin (the spot light of the built-in scene's run).
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

template <typename F>
static bool throws_invalid(F f)
{
    try { f(); } catch (const CrychicException& e) { return e.Status == CRYCHIC_E_INVALID_ARG; }
    return false;
}

int main(int argc, char** argv)
{
    if (argc < 10) { std::fprintf(stderr, "usage\n"); return 2; }
    const std::string dir = argv[1];
    const UINT W = std::atoi(argv[2]), H = std::atoi(argv[3]), SD = std::atoi(argv[4]), CD = std::atoi(argv[5]);
    const uint32_t count = std::atoi(argv[8]), dim = std::atoi(argv[9]);
    const float fovY = 1.5707964f, zNear = 0.5f;
    try {
        GameTimer gt;
        auto frame = [&](CRYCHIC& app, const std::string& name) {
            for (int f = 0; f < 4; ++f) {               // cycles the frame-resource ring
                gt.Tick(1.0f / 60.0f);
                app.Update(gt);
                app.Draw(gt);
            }
            app.CommandList()->Flush();
            std::vector<uint8_t> out((size_t)W * H * 4);
            hipStream_t s = app.CommandList()->Stream();
            app.CurrentBackBuffer()->Download(out.data(), out.size(), s);
            app.CommandList()->Flush();
            dump(dir + "/" + name, out.data(), out.size());
        };
        {
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

            const std::vector<Light> spots = lights(dir + "/spots.bin");
            app.SetLocalLights(nullptr, 0, spots.data(), (uint32_t)spots.size());
            // errors throw CrychicException, as everywhere in the veneer, and leave the shadows as they were (none)
            const uint32_t n = (uint32_t)spots.size();
            const bool errs = throws_invalid([&] { app.SetSpotShadows(9, dim, fovY, zNear); }) &&
                              throws_invalid([&] { app.SetSpotShadows(n + 1, dim, fovY, zNear); }) &&
                              throws_invalid([&] { app.SetSpotShadows(count, 1, fovY, zNear); }) &&
                              throws_invalid([&] { app.SetSpotShadows(count, 16385, fovY, zNear); }) &&
                              throws_invalid([&] { app.SetSpotShadows(count, dim, 0.0f, zNear); }) &&
                              throws_invalid([&] { app.SetSpotShadows(count, dim, 3.2f, zNear); }) &&
                              throws_invalid([&] { app.SetSpotShadows(count, dim, fovY, 0.0f); }) &&
                              throws_invalid([&] { app.SetSpotShadows(count, dim, fovY, 1.0e6f); });
            if (!errs || app.SpotShadowMap(0)) { std::fprintf(stderr, "SetSpotShadows argument errors not reported\n"); return 4; }

            app.SetSpotShadows(count, dim, fovY, zNear);
            for (uint32_t k = 0; k < count; ++k) put(app.SpotShadowMap(k), dir + "/spotmap" + std::to_string(k) + ".bin", s);
            frame(app, "out.bin");
            dump(dir + "/pass_cb.bin", &app.mCurrFrameResource->PassCB->Element(0), sizeof(PassConstants));
            dump(dir + "/ssao_cb.bin", &app.mCurrFrameResource->SsaoCB->Element(0), sizeof(SsaoConstants));
            app.SetSpotShadows(0, 0, 0.0f, 0.0f);          // the unshadowed spot lights again
            frame(app, "out_noshadow.bin");
        }
        {
            // the built-in scene with its producer passes: the spot maps are rendered after the cascades
            CRYCHIC app(0, W, H);
            app.mShadowMapSize = SD;
            app.mBlurCount = std::atoi(argv[6]);
            app.mNumDirLights = 1;
            app.mSkyEnabled = true;
            if (!app.Initialize()) return 3;
            auto cube = std::make_unique<ID3D12Resource>((size_t)6 * CD * CD * 4, ID3D12Resource::DEFAULT_HEAP);
            put(cube.get(), dir + "/cube.bin", app.CommandList()->Stream());
            app.SetCubeMap(std::move(cube), CD);
            const std::vector<Light> spots = lights(dir + "/scene_spots.bin");
            app.SetLocalLights(nullptr, 0, spots.data(), (uint32_t)spots.size());
            app.SetSpotShadows((uint32_t)spots.size(), 1024, fovY, zNear);
            frame(app, "scene_shadowed.bin");
            std::vector<uint32_t> m((size_t)1024 * 1024);
            app.SpotShadowMap(0)->Download(m.data(), m.size() * 4, app.CommandList()->Stream());
            app.CommandList()->Flush();
            dump(dir + "/scene_spotmap0.bin", m.data(), m.size() * 4);
            app.SetSpotShadows(0, 0, 0.0f, 0.0f);
            frame(app, "scene_unshadowed.bin");
        }
        std::printf("spot shadow driver ok %ux%u\n", W, H);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
