// point_shadows_driver.cpp -- the C++ veneer's shadowed point lights, as a reference call site would drive them (Update / Draw); frames
// go back for comparison with the Python path (tests/test_point_shadows_veneer.py).  Two runs:
//   1. point lights with SetPointShadows(<count>, <dim>, 0.5) and the caller's faces: out_point.bin (pass_cb_point.bin,
//      ssao_cb_point.bin), then SetPointShadows(0): out_point_none.bin;
//   2. the built-in scene with its producer passes and one shadowed point light: scene_point.bin, scene_pointmap0.bin (six faces of
//      256), scene_point_none.bin.
// Usage: point_shadows_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights> <count> <dim>
// <dir> holds the planes veneer_driver reads, points.bin (an array of Light), pointmap<k>.bin (six dim x dim D24 faces of the first
// <count> point lights) and scene_points.bin (the point light of run 2).
#include <cstring>
#include "driver_util.hpp"

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
    const float zNear = 0.5f;
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
            app.CurrentBackBuffer()->Download(out.data(), out.size(), app.CommandList()->Stream());
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
            const std::vector<Light> points = lights(dir + "/points.bin");
            app.SetLocalLights(points.data(), (uint32_t)points.size(), nullptr, 0);
            // errors throw CrychicException, as everywhere in the veneer, and leave the shadows as they were (none)
            const uint32_t n = (uint32_t)points.size();
            const bool errs = throws_invalid([&] { app.SetPointShadows(5, dim, zNear); }) &&
                              (n >= 4 || throws_invalid([&] { app.SetPointShadows(n + 1, dim, zNear); })) &&
                              throws_invalid([&] { app.SetPointShadows(count, 15, zNear); }) &&
                              throws_invalid([&] { app.SetPointShadows(count, 16385, zNear); }) &&
                              throws_invalid([&] { app.SetPointShadows(count, dim, 0.0f); }) &&
                              throws_invalid([&] { app.SetPointShadows(count, dim, 1.0e6f); });
            if (!errs || app.PointShadowMap(0)) { std::fprintf(stderr, "SetPointShadows argument errors not reported\n"); return 4; }
            app.SetPointShadows(count, dim, zNear);
            for (uint32_t k = 0; k < count; ++k) put(app.PointShadowMap(k), dir + "/pointmap" + std::to_string(k) + ".bin", s);
            frame(app, "out_point.bin");
            dump(dir + "/pass_cb_point.bin", &app.mCurrFrameResource->PassCB->Element(0), sizeof(PassConstants));
            dump(dir + "/ssao_cb_point.bin", &app.mCurrFrameResource->SsaoCB->Element(0), sizeof(SsaoConstants));
            app.SetPointShadows(0, 0, 0.0f);                // the unshadowed point lights again
            frame(app, "out_point_none.bin");
        }
        {
            // the built-in scene with its producer passes: the faces are rendered after the cascades
            CRYCHIC app(0, W, H);
            app.mShadowMapSize = SD;
            app.mBlurCount = std::atoi(argv[6]);
            app.mNumDirLights = 1;
            app.mSkyEnabled = true;
            if (!app.Initialize()) return 3;
            auto cube = std::make_unique<ID3D12Resource>((size_t)6 * CD * CD * 4, ID3D12Resource::DEFAULT_HEAP);
            put(cube.get(), dir + "/cube.bin", app.CommandList()->Stream());
            app.SetCubeMap(std::move(cube), CD);
            const std::vector<Light> points = lights(dir + "/scene_points.bin");
            app.SetLocalLights(points.data(), (uint32_t)points.size(), nullptr, 0);
            app.SetPointShadows((uint32_t)points.size(), 256, zNear);
            frame(app, "scene_point.bin");
            std::vector<uint32_t> m((size_t)6 * 256 * 256);
            app.PointShadowMap(0)->Download(m.data(), m.size() * 4, app.CommandList()->Stream());
            app.CommandList()->Flush();
            dump(dir + "/scene_pointmap0.bin", m.data(), m.size() * 4);
            app.SetPointShadows(0, 0, 0.0f);
            frame(app, "scene_point_none.bin");
        }
        std::printf("point shadows driver ok %ux%u\n", W, H);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
