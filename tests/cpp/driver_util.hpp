// driver_util.hpp -- what the drivers of tests/cpp share: slurp and dump, and for the drivers of the post-process passes the application
// they all set up the same way (run_post_driver) with its frame() and grab().
#pragma once
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>
#include "crychic/CRYCHIC.h"

inline std::vector<char> slurp(const std::string& p)
{
    std::ifstream f(p, std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", p.c_str()); std::exit(2); }
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
inline void dump(const std::string& p, const void* d, size_t n)
{
    std::ofstream f(p, std::ios::binary);
    f.write(static_cast<const char*>(d), (std::streamsize)n);
}

// What run_post_driver hands the driver's body: the initialized application over its built-in scene, its stream and its timer.
struct PostDriver {
    const std::string dir;
    const UINT W, H;
    CRYCHIC& app;
    hipStream_t s;
    GameTimer gt;

    // one frame: Update and Draw, waited for
    void frame() { gt.Tick(1.0f / 60.0f); app.Update(gt); app.Draw(gt); app.CommandList()->Flush(); }
    // the resource's bytes into <dir>/<name>
    void grab(ID3D12Resource* r, const std::string& name)
    {
        std::vector<char> h(r->Bytes());
        r->Download(h.data(), h.size(), s);
        app.CommandList()->Flush();
        dump(dir + "/" + name, h.data(), h.size());
    }
};

// main() of a driver called as <driver> <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights> [more, minArgs counts them]:
// a W x H application with the producer passes and the sky on, initialized, the cube map of <dir>/cube.bin set; then body(PostDriver&),
// whose value is the exit code.  2: usage or a bad file, 3: Initialize failed, 1: an exception.
template <class Body>
int run_post_driver(int argc, char** argv, Body body, int minArgs = 8)
{
    if (argc < minArgs) { std::fprintf(stderr, "usage\n"); return 2; }
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
        auto cubeBytes = slurp(dir + "/cube.bin");
        auto cube = std::make_unique<ID3D12Resource>((size_t)6 * CD * CD * 4, ID3D12Resource::DEFAULT_HEAP);
        if (cubeBytes.size() != cube->Bytes()) { std::fprintf(stderr, "cube.bin size\n"); return 2; }
        cube->Upload(cubeBytes.data(), cubeBytes.size(), s);
        CrychicHipThrowIfFailed(hipStreamSynchronize(s));
        app.SetCubeMap(std::move(cube), CD);
        PostDriver d{dir, W, H, app, s, GameTimer()};
        return body(d);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
