// env_capture_driver.cpp -- the C++ veneer's environment capture (include/crychic/CRYCHIC.h CaptureEnvironment), as a reference call
// site would drive it; the captured chain and the frame rendered with it go back for comparison with the Python path
// (tests/test_env_capture_veneer.py).  The built-in scene with its producer passes, frustum culling off (the Python path draws
// every instance): one frame, CaptureEnvironment(x, y, z, dim, levels, captureShadowDim), chain.bin (the bound chain), then a
// frame with the captured chain bound: out.bin, pass_cb.bin, ssao_cb.bin.
// Usage: env_capture_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <dim> <levels> <captureShadowDim> <x> <y> <z> [lights]
// <dir> holds cube.bin, the one-level source cube map of <cubeDim>; with `lights` also points.bin and spots.bin (arrays of Light):
// SetLocalLights with both and SetSpotShadows(1, 128, pi / 2, 0.5), so that the probe reads this object's lights and shadow map.
#include <cstring>
#include "driver_util.hpp"

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
    if (argc < 13) { std::fprintf(stderr, "usage\n"); return 2; }
    const std::string dir = argv[1];
    const UINT W = std::atoi(argv[2]), H = std::atoi(argv[3]), SD = std::atoi(argv[4]), CD = std::atoi(argv[5]);
    const UINT dim = std::atoi(argv[7]), levels = std::atoi(argv[8]), captureSD = std::atoi(argv[9]);
    const float x = (float)std::atof(argv[10]), y = (float)std::atof(argv[11]), z = (float)std::atof(argv[12]);
    try {
        GameTimer gt;
        CRYCHIC app(0, W, H);
        app.mShadowMapSize = SD;
        app.mBlurCount = std::atoi(argv[6]);
        app.mNumDirLights = 1;
        app.mSkyEnabled = true;
        app.mFrustumCullingEnabled = false;
        if (!app.Initialize()) return 3;
        hipStream_t s = app.CommandList()->Stream();
        // a capture needs a source
        if (!throws_invalid([&] { app.CaptureEnvironment(x, y, z, dim, levels, captureSD); })) { std::fprintf(stderr, "capture without a source not refused\n"); return 4; }
        auto cube = std::make_unique<ID3D12Resource>((size_t)6 * CD * CD * 4, ID3D12Resource::DEFAULT_HEAP);
        auto b = slurp(dir + "/cube.bin");
        if (b.size() != cube->Bytes()) { std::fprintf(stderr, "cube.bin: %zu bytes, expected %zu\n", b.size(), cube->Bytes()); return 2; }
        cube->Upload(b.data(), b.size(), s);
        app.CommandList()->Flush();
        const void* source = cube->Data();
        app.SetCubeMap(std::move(cube), CD);
        if (argc > 13 && std::string(argv[13]) == "lights") {
            const std::vector<Light> points = lights(dir + "/points.bin"), spots = lights(dir + "/spots.bin");
            app.SetLocalLights(points.data(), (uint32_t)points.size(), spots.data(), (uint32_t)spots.size());
            app.SetSpotShadows(1, 128, (float)(3.14159265358979323846 / 2.0), 0.5f);
            // shadowed local lights: the probe reads this object's maps, which need a frame's instance buffers to be rendered
            if (!throws_invalid([&] { app.CaptureEnvironment(x, y, z, dim, levels, captureSD); })) { std::fprintf(stderr, "capture before Update not refused\n"); return 4; }
        }
        auto frame = [&] {
            gt.Tick(1.0f / 60.0f);
            app.Update(gt);
            app.Draw(gt);
            app.CommandList()->Flush();
        };
        frame();
        const bool errs = throws_invalid([&] { app.CaptureEnvironment(x, y, z, dim + 1, 0, captureSD); }) &&
                          throws_invalid([&] { app.CaptureEnvironment(x, y, z, 0, 0, captureSD); }) &&
                          throws_invalid([&] { app.CaptureEnvironment(x, y, z, dim, 16, captureSD); });
        if (!errs || app.CubeMap()->Data() != source) { std::fprintf(stderr, "CaptureEnvironment argument errors not reported\n"); return 4; }
        app.mRunProducerPasses = false;        // caller-filled planes: no scene to capture
        const bool refused = throws_invalid([&] { app.CaptureEnvironment(x, y, z, dim, levels, captureSD); });
        app.mRunProducerPasses = true;
        if (!refused) { std::fprintf(stderr, "capture of caller-filled planes not refused\n"); return 4; }
        app.CaptureEnvironment(x, y, z, dim, levels, captureSD);
        if (app.CubeMap()->Data() == source || app.CubeMapSize() != dim) { std::fprintf(stderr, "the captured chain is not bound\n"); return 5; }
        std::vector<uint8_t> chain(app.CubeMap()->Bytes());
        app.CubeMap()->Download(chain.data(), chain.size(), s);
        app.CommandList()->Flush();
        dump(dir + "/chain.bin", chain.data(), chain.size());
        frame();
        std::vector<uint8_t> out((size_t)W * H * 4);
        app.CurrentBackBuffer()->Download(out.data(), out.size(), s);
        app.CommandList()->Flush();
        dump(dir + "/out.bin", out.data(), out.size());
        dump(dir + "/pass_cb.bin", &app.mCurrFrameResource->PassCB->Element(0), sizeof(PassConstants));
        dump(dir + "/ssao_cb.bin", &app.mCurrFrameResource->SsaoCB->Element(0), sizeof(SsaoConstants));
        std::printf("env capture driver ok dim %u levels %u\n", dim, app.CubeMapLevels());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
