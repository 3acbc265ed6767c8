// post_chain_driver.cpp -- the passes behind the lighting pass as CRYCHIC::Draw chains them (include/crychic/CRYCHIC.h):
//     lighting -> fog (in place) -> temporal anti-aliasing -> depth of field -> motion blur -> bloom -> anti-aliasing.
// For each subset of the six switches with at most two of the five buffered stages, or all five, with and without the fog (bit k of
// the mask = the k-th switch in the order above), the application's built-in scene is drawn twice from the home camera, which strafes
// before the second frame.  Frame k of mask m leaves back_m_k.bin (the back buffer), depth_m_k.bin, cb_m_k.bin (the frame's pass
// constants, InvViewProj among them), mats_m_k.bin (the unjittered ViewProj pairs of the temporal pass and of the motion blur: 64
// floats), every set stage's buffer (taa_, hist_, dof_, mb_, bloom_, aa_) and present_m_k.ppm (what Present writes).  At the end all
// switches are off again (plain_again.bin).  tests/test_post_chain_veneer.py applies each pass to the buffer in front of it.
// Usage: post_chain_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include <cstring>
#include "driver_util.hpp"

enum { FOG = 1, TAA = 2, DOF = 4, MB = 8, BLOOM = 16, AA = 32, ALL = 63 };

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [](PostDriver& d) {
        CRYCHIC& app = d.app;
        const std::string& dir = d.dir;
        crychic_bloom_params glow;                              // a threshold the scene's highlights pass (the test states the same numbers)
        crychic_bloom_default_params(&glow);
        glow.threshold = 160; glow.knee = 32; glow.scatter = 179; glow.intensity = 64; glow.levels = 6;
        auto set = [&](int mask) {
            app.SetFog((mask & FOG) != 0);
            app.SetTemporalAA((mask & TAA) != 0);
            app.SetDepthOfField((mask & DOF) != 0);
            app.SetMotionBlur((mask & MB) != 0);
            app.SetBloom((mask & BLOOM) != 0, &glow);
            app.SetAntiAliasing((mask & AA) != 0);
        };
        const DirectX::XMFLOAT3 home = app.mCamera.GetPosition3f();
        int drawn = 0;
        for (int mask = 0; mask <= ALL; ++mask) {
            int stages = 0;
            for (int b = TAA; b <= AA; b <<= 1) stages += (mask & b) != 0;
            if (stages > 2 && stages != 5) continue;
            set(0);                                             // from cleared: a reset frame, no previous camera
            set(mask);
            app.mCamera.SetPosition(home.x, home.y, home.z);
            for (int k = 0; k < 2; ++k) {
                if (k) app.mCamera.Strafe(0.3f);
                d.frame();
                const std::string tag = "_" + std::to_string(mask) + "_" + std::to_string(k);
                d.grab(app.CurrentBackBuffer(), "back" + tag + ".bin");
                d.grab(app.DepthStencilBuffer(), "depth" + tag + ".bin");
                dump(dir + "/cb" + tag + ".bin", &app.mMainPassCB, sizeof app.mMainPassCB);
                float m[64];
                std::memcpy(m, app.TemporalAAViewProj(0), 64);
                std::memcpy(m + 16, app.TemporalAAViewProj(1), 64);
                std::memcpy(m + 32, app.MotionBlurViewProj(0), 64);
                std::memcpy(m + 48, app.MotionBlurViewProj(1), 64);
                dump(dir + "/mats" + tag + ".bin", m, sizeof m);
                if (mask & TAA) { d.grab(app.TemporalAABackBuffer(), "taa" + tag + ".bin"); d.grab(app.TemporalAAHistory(), "hist" + tag + ".bin"); }
                if (mask & DOF) d.grab(app.DepthOfFieldBackBuffer(), "dof" + tag + ".bin");
                if (mask & MB) d.grab(app.MotionBlurBackBuffer(), "mb" + tag + ".bin");
                if (mask & BLOOM) d.grab(app.BloomBackBuffer(), "bloom" + tag + ".bin");
                if (mask & AA) d.grab(app.AntiAliasedBackBuffer(), "aa" + tag + ".bin");
                app.Present(dir + "/present" + tag + ".ppm");
            }
            ++drawn;
        }
        set(0);
        app.mCamera.SetPosition(home.x, home.y, home.z);
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("post chain driver ok %ux%u, %d subsets\n", d.W, d.H, drawn);
        return 0;
    });
}
