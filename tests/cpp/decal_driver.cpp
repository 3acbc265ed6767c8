// decal_driver.cpp -- CRYCHIC::SetDecals / ClearDecals through the C++ veneer (include/crychic/CRYCHIC.h): the application's built-in
// scene is drawn without decals (plain.bin = the back buffer; g0.bin .. g2.bin, depth.bin and pass_cb.bin = what the pass reads), then
// with the decals of decals.bin over the texture chain of tex.bin (decal.bin = the back buffer, g0_decal.bin .. g2_decal.bin = the
// planes), then cleared (plain_again.bin), then with the decals as a strip of the frame (g1_strip.bin: the strip's rows decaled, the
// others as the plain frame left them); too many decals must be refused (tests/test_decal_veneer.py).
// Usage: decal_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights> <texW> <texH> <texLevels> <strip row0> <strip rows>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [argv](PostDriver& d) {
        CRYCHIC& app = d.app;
        const std::string& dir = d.dir;
        const UINT W = d.W, H = d.H;
        const UINT texW = std::atoi(argv[8]), texH = std::atoi(argv[9]), texLevels = std::atoi(argv[10]), stripRow0 = std::atoi(argv[11]), stripRows = std::atoi(argv[12]);
        if (app.DecalCount() != 0) { std::fprintf(stderr, "decals are set by default\n"); return 4; }
        auto texBytes = slurp(dir + "/tex.bin");
        auto tex = std::make_unique<ID3D12Resource>(texBytes.size(), ID3D12Resource::DEFAULT_HEAP);
        tex->Upload(texBytes.data(), texBytes.size(), d.s);
        CrychicHipThrowIfFailed(hipStreamSynchronize(d.s));
        auto decalBytes = slurp(dir + "/decals.bin");
        const uint32_t n = (uint32_t)(decalBytes.size() / sizeof(crychic_decal));
        const crychic_decal* decals = reinterpret_cast<const crychic_decal*>(decalBytes.data());
        const crychic_texture table[1] = { { static_cast<const uint8_t*>(tex->Data()), texW, texH, texLevels } };

        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");
        d.grab(app.DepthStencilBuffer(), "depth.bin");
        for (int i = 0; i < 3; ++i) d.grab(app.mDeferred->Resource(i), "g" + std::to_string(i) + ".bin");
        dump(dir + "/pass_cb.bin", &app.mMainPassCB, sizeof app.mMainPassCB);

        // more decals than the pass takes are refused and leave none set
        int refused = 0;
        std::vector<crychic_decal> many(CRYCHIC_MAX_DECALS + 1, decals[0]);
        try { app.SetDecals(many.data(), (uint32_t)many.size(), table, 1); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 1 || app.DecalCount() != 0) { std::fprintf(stderr, "too many decals were not refused\n"); return 5; }

        app.SetDecals(decals, n, table, 1);
        if (app.DecalCount() != n) { std::fprintf(stderr, "SetDecals\n"); return 6; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "decal.bin");
        for (int i = 0; i < 3; ++i) d.grab(app.mDeferred->Resource(i), "g" + std::to_string(i) + "_decal.bin");

        app.ClearDecals();
        if (app.DecalCount() != 0) { std::fprintf(stderr, "ClearDecals\n"); return 7; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");

        // a strip: the producers and the decals touch its rows alone
        app.SetDecals(decals, n, table, 1);
        app.SetStrip(stripRow0, stripRows);
        d.frame();
        d.grab(app.mDeferred->Resource(1), "g1_strip.bin");
        app.SetWholeFrame();
        std::printf("decal driver ok %ux%u %u decals\n", W, H, n);
        return 0;
    }, 13);
}
