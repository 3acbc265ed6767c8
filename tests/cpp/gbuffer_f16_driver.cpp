// gbuffer_f16_driver.cpp -- the G-buffer plane formats through the C++ veneer (include/crychic/DeferredShading.h, CRYCHIC.h), as a
// reference call site would use them: DeferredShading built with DXGI_FORMAT_R16G16B16A16_FLOAT and with a format per plane,
// CRYCHIC::SetGBufferFormat followed by Update / Draw on the application's built-in scene (producer passes included), and the
// refusal of any other format.  The planes and the back buffer go back as raw files (tests/test_gbuffer_f16_gpu.py).
// Usage: gbuffer_f16_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights> <f32|mixed|f16>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    if (argc < 9) { std::fprintf(stderr, "usage\n"); return 2; }
    const std::string dir = argv[1], mix = argv[8];
    const UINT W = std::atoi(argv[2]), H = std::atoi(argv[3]), SD = std::atoi(argv[4]), CD = std::atoi(argv[5]);
    const DXGI_FORMAT F32 = DXGI_FORMAT_R32G32B32A32_FLOAT, F16 = DXGI_FORMAT_R16G16B16A16_FLOAT;
    try {
        CRYCHIC app(0, W, H);
        app.mShadowMapSize = SD;
        app.mBlurCount = std::atoi(argv[6]);
        app.mNumDirLights = std::atoi(argv[7]);
        app.mSkyEnabled = true;
        app.mRunProducerPasses = true;
        if (!app.Initialize()) return 3;
        hipStream_t s = app.CommandList()->Stream();
        if (app.mDeferred->FormatFlags() != 0u || app.mDeferred->Format() != F32) { std::fprintf(stderr, "the default is not R32G32B32A32\n"); return 4; }

        {   // the pass object on its own: one format for all planes, a format per plane, each plane at its own size
            DeferredShading all(app.Device(), W, H, F16);
            const DXGI_FORMAT per[3] = { F32, F16, F32 };
            DeferredShading some(app.Device(), W, H, per);
            const size_t n = (size_t)W * H;
            const bool ok = all.FormatFlags() == CRYCHIC_GBUFFER_F16_MASK && all.Format(0) == F16 && all.Format(2) == F16 &&
                            all.Resource(0)->Bytes() == n * 8 && all.Resource(2)->Bytes() == n * 8 &&
                            some.FormatFlags() == CRYCHIC_GBUFFER_G1_F16 && some.Format(0) == F32 && some.Format(1) == F16 &&
                            some.Resource(0)->Bytes() == n * 16 && some.Resource(1)->Bytes() == n * 8 && some.Resource(2)->Bytes() == n * 16;
            if (!ok) { std::fprintf(stderr, "DeferredShading formats / plane sizes\n"); return 5; }
        }
        // any other format is still refused, by the pass object and by the application
        int refused = 0;
        try { DeferredShading bad(app.Device(), W, H, DXGI_FORMAT_R8G8B8A8_UNORM); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_UNSUPPORTED; }
        try { app.SetGBufferFormat(F32, DXGI_FORMAT_R24G8_TYPELESS, F16); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_UNSUPPORTED; }
        if (refused != 2 || app.mDeferred->FormatFlags() != 0u) { std::fprintf(stderr, "an unsupported format was not refused\n"); return 6; }

        if (mix == "mixed") app.SetGBufferFormat(F32, F16, F16);
        else if (mix == "f16") app.SetGBufferFormat(F16, F16, F16);
        else if (mix != "f32") { std::fprintf(stderr, "unknown mix %s\n", mix.c_str()); return 2; }

        auto cubeBytes = slurp(dir + "/cube.bin");
        auto cube = std::make_unique<ID3D12Resource>((size_t)6 * CD * CD * 4, ID3D12Resource::DEFAULT_HEAP);
        if (cubeBytes.size() != cube->Bytes()) { std::fprintf(stderr, "cube.bin size\n"); return 2; }
        cube->Upload(cubeBytes.data(), cubeBytes.size(), s);
        CrychicHipThrowIfFailed(hipStreamSynchronize(s));
        app.SetCubeMap(std::move(cube), CD);

        GameTimer gt;
        for (int frame = 0; frame < 3; ++frame) {
            gt.Tick(1.0f / 60.0f);
            app.Update(gt);
            if (frame == 1) app.mFuseCameraPasses = false;       // the separate passes take the formats as well: same planes, same frame
            app.Draw(gt);
        }
        app.CommandList()->Flush();
        auto grab = [&](ID3D12Resource* r, const std::string& name) {
            std::vector<char> h(r->Bytes());
            r->Download(h.data(), h.size(), s);
            app.CommandList()->Flush();
            dump(dir + "/" + name, h.data(), h.size());
        };
        grab(app.CurrentBackBuffer(), "out.bin");
        grab(app.mSsao->AmbientMap(), "ao.bin");
        grab(app.DepthStencilBuffer(), "depth_out.bin");
        grab(app.mSsao->NormalMap(), "normal_out.bin");
        for (int i = 0; i < 3; ++i) grab(app.mDeferred->Resource(i), "g" + std::to_string(i) + "_out.bin");
        for (int i = 0; i < 4; ++i) grab(app.mShadowMap->Resource(i), "shadow" + std::to_string(i) + "_out.bin");
        dump(dir + "/pass_cb.bin", &app.mCurrFrameResource->PassCB->Element(0), sizeof(PassConstants));
        dump(dir + "/ssao_cb.bin", &app.mCurrFrameResource->SsaoCB->Element(0), sizeof(SsaoConstants));
        std::printf("gbuffer f16 driver ok %ux%u %s flags 0x%x\n", W, H, mix.c_str(), app.mDeferred->FormatFlags());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
