// env_ambient_driver.cpp -- the C++ veneer's ambient light from the environment (include/crychic/CRYCHIC.h SetEnvironmentAmbient), as a
// reference call site would drive it; the captured chain with its environment tail and the frame rendered with it go back for
// comparison with the Python path (tests/test_env_ambient_veneer.py).  The built-in scene with its producer passes, frustum culling
// off (the Python path draws every instance): SetEnvironmentAmbient(true), with <gloss> 1 SetGlossyReflections(true) and the full
// chain, with 0 level 0 alone; one frame, CaptureEnvironment(x, y, z, dim, levels, captureShadowDim), chain.bin (the bound cube map
// and its tail), then a frame with it bound: out.bin, pass_cb.bin, ssao_cb.bin.
// Usage: env_ambient_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <dim> <captureShadowDim> <x> <y> <z> <gloss>
// <dir> holds cube.bin, the one-level source cube map of <cubeDim>.
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    if (argc < 13) { std::fprintf(stderr, "usage\n"); return 2; }
    const std::string dir = argv[1];
    const UINT W = std::atoi(argv[2]), H = std::atoi(argv[3]), SD = std::atoi(argv[4]), CD = std::atoi(argv[5]);
    const UINT dim = std::atoi(argv[7]), captureSD = std::atoi(argv[8]);
    const float x = (float)std::atof(argv[9]), y = (float)std::atof(argv[10]), z = (float)std::atof(argv[11]);
    const bool gloss = std::atoi(argv[12]) != 0;
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
        auto cube = std::make_unique<ID3D12Resource>((size_t)6 * CD * CD * 4, ID3D12Resource::DEFAULT_HEAP);
        auto b = slurp(dir + "/cube.bin");
        if (b.size() != cube->Bytes()) { std::fprintf(stderr, "cube.bin: %zu bytes, expected %zu\n", b.size(), cube->Bytes()); return 2; }
        cube->Upload(b.data(), b.size(), s);
        app.CommandList()->Flush();
        app.SetCubeMap(std::move(cube), CD);
        app.SetGlossyReflections(gloss);
        app.SetEnvironmentAmbient(true);
        if (!app.EnvironmentAmbient() || app.CubeMapHasTail()) return 4;
        auto frame = [&] {
            gt.Tick(1.0f / 60.0f);
            app.Update(gt);
            app.Draw(gt);           // before the capture the bound cube map has no tail: the constant ambient term
            app.CommandList()->Flush();
        };
        frame();
        app.CaptureEnvironment(x, y, z, dim, gloss ? 0 : 1, captureSD);
        if (!app.CubeMapHasTail() || app.CubeMap()->Bytes() != crychic_cube_chain_sh_bytes(dim, app.CubeMapLevels())) return 5;
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
        std::printf("env ambient driver ok dim %u levels %u\n", dim, app.CubeMapLevels());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
