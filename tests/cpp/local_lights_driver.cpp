// local_lights_driver.cpp -- the C++ veneer's local lights, as a reference call site would drive them (Update / Draw); frames go
// back for comparison with the Python path (tests/test_spot_lights.py, tests/test_spot_shadows_veneer.py).  Three runs:
//   1. CRYCHIC::SetLocalLights with point and spot lists: out.bin, then cleared to nothing: out_nolights.bin (pass_cb.bin, ssao_cb.bin);
//   2. spot lights with SetSpotShadows(<count>, <dim>) and the caller's maps: out_shadowed.bin, then SetSpotShadows(0):
//      out_noshadow.bin (pass_cb_shadowed.bin, ssao_cb_shadowed.bin);
//   3. the built-in scene with its producer passes and one shadowed spot light: scene_shadowed.bin, scene_spotmap0.bin,
//      scene_unshadowed.bin.
// Usage: local_lights_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights> <count> <dim>
// <dir> holds the planes veneer_driver reads, points.bin and spots.bin (arrays of Light), randvec.bin (run 2's random-vector map),
// spotmap<k>.bin (the first <count> maps, dim x dim D24) and scene_spots.bin (the spot light of run 3).
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
        auto dump_cbs = [&](CRYCHIC& app, const std::string& suffix) {
            dump(dir + "/pass_cb" + suffix + ".bin", &app.mCurrFrameResource->PassCB->Element(0), sizeof(PassConstants));
            dump(dir + "/ssao_cb" + suffix + ".bin", &app.mCurrFrameResource->SsaoCB->Element(0), sizeof(SsaoConstants));
        };
        // an app over the planes of <dir> (no producer passes)
        auto with_planes = [&](CRYCHIC& app) {
            app.mShadowMapSize = SD;
            app.mBlurCount = std::atoi(argv[6]);
            app.mNumDirLights = std::atoi(argv[7]);
            app.mSkyEnabled = true;
            app.mRunProducerPasses = false;
            if (!app.Initialize()) return false;
            hipStream_t s = app.CommandList()->Stream();
            put(app.DepthStencilBuffer(), dir + "/depth.bin", s);
            put(app.mSsao->NormalMap(), dir + "/normal.bin", s);
            for (int i = 0; i < 3; ++i) put(app.mDeferred->Resource(i), dir + "/g" + std::to_string(i) + ".bin", s);
            for (int i = 0; i < 4; ++i) put(app.mShadowMap->Resource(i), dir + "/shadow" + std::to_string(i) + ".bin", s);
            auto cube = std::make_unique<ID3D12Resource>((size_t)6 * CD * CD * 4, ID3D12Resource::DEFAULT_HEAP);
            put(cube.get(), dir + "/cube.bin", s);
            app.SetCubeMap(std::move(cube), CD);
            return true;
        };
        const std::vector<Light> points = lights(dir + "/points.bin"), spots = lights(dir + "/spots.bin");
        {
            CRYCHIC app(0, W, H);
            if (!with_planes(app)) return 3;
            // errors throw CrychicException, as everywhere in the veneer
            if (!throws_invalid([&] { app.SetLocalLights(nullptr, 1, nullptr, 0); })) {
                std::fprintf(stderr, "SetLocalLights(nullptr, 1) did not throw\n");
                return 4;
            }
            std::vector<Light> many(1025);
            if (!throws_invalid([&] { app.SetLocalLights(nullptr, 0, many.data(), 1025); })) {
                std::fprintf(stderr, "SetLocalLights(1025 spots) did not throw\n");
                return 4;
            }
            app.SetLocalLights(points.data(), (uint32_t)points.size(), spots.data(), (uint32_t)spots.size());
            frame(app, "out.bin");
            app.SetLocalLights(nullptr, 0, nullptr, 0);     // today's behaviour again
            frame(app, "out_nolights.bin");
            dump_cbs(app, "");
        }
        {
            CRYCHIC app(0, W, H);
            if (!with_planes(app)) return 3;
            hipStream_t s = app.CommandList()->Stream();
            // the veneer draws its random-vector map from the process-wide rand() state (Ssao::RandState), which run 1 has advanced:
            // this run takes the map a fresh process builds
            put(app.mSsao->RandomVectorMap(), dir + "/randvec.bin", s);
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
            frame(app, "out_shadowed.bin");
            dump_cbs(app, "_shadowed");
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
        std::printf("local lights driver ok %ux%u\n", W, H);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
