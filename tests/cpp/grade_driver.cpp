// grade_driver.cpp -- CRYCHIC::SetColourGrade, SetColourGradeLut and LoadColourGradeLut through the C++ veneer
// (include/crychic/CRYCHIC.h): the application's built-in scene is drawn with the stage off (plain.bin = the back buffer), then with
// the table of an ASC CDL (grade_frame.bin = the back buffer, grade_cdl.bin = the stage's buffer), with the caller's table of
// <dir>/lut5.bin (grade_lut5.bin), with the file <dir>/look.cube (grade_cube.bin), together with SetBloom and SetAntiAliasing
// (grade_bloom_in.bin = the bloom buffer the stage read, grade_bloom.bin = the stage's buffer, grade_bloom_aa.bin = the anti-aliased
// buffer), then off again (plain_again.bin); what is refused must leave the stage as it was, and a strip with it on must make Draw
// throw (tests/test_grade_veneer.py).
// Usage: grade_driver <dir> <W> <H> <shadowDim> <cubeDim> <blurCount> <numDirLights>
#include "driver_util.hpp"

int main(int argc, char** argv)
{
    return run_post_driver(argc, argv, [](PostDriver& d) {
        CRYCHIC& app = d.app;
        const UINT W = d.W, H = d.H;
        if (app.ColourGrade() || app.ColourGradeBackBuffer()) { std::fprintf(stderr, "the colour grade is on by default\n"); return 4; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain.bin");

        // the look tests/test_grade_veneer.py states
        crychic_grade_params warm;
        crychic_grade_default_params(&warm);
        warm.slope[0] = 1.2f; warm.slope[2] = 0.8f;
        warm.offset[0] = 0.03f; warm.offset[2] = -0.02f;
        warm.power[0] = 0.9f; warm.power[2] = 1.2f;
        warm.saturation = 1.3f;
        app.SetColourGrade(&warm);
        if (!app.ColourGrade() || !app.ColourGradeBackBuffer() || app.ColourGradeSize() != CRYCHIC_GRADE_MAX_N) { std::fprintf(stderr, "SetColourGrade\n"); return 5; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "grade_frame.bin");
        d.grab(app.ColourGradeBackBuffer(), "grade_cdl.bin");

        // what is refused leaves the stage as it was
        int refused = 0;
        crychic_grade_params bad = warm;
        bad.saturation = 9.0f;
        try { app.SetColourGrade(&bad); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        const std::vector<char> lut5 = slurp(d.dir + "/lut5.bin");
        try { app.SetColourGradeLut(reinterpret_cast<const uint8_t*>(lut5.data()), 34); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        try { app.SetColourGradeLut(reinterpret_cast<const uint8_t*>(lut5.data()), 1); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        try { app.LoadColourGradeLut((d.dir + "/missing.cube").c_str()); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        try { app.LoadColourGradeLut((d.dir + "/one_d.cube").c_str()); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_UNSUPPORTED; }
        if (refused != 5 || !app.ColourGrade() || app.ColourGradeSize() != CRYCHIC_GRADE_MAX_N) { std::fprintf(stderr, "a bad table was not refused\n"); return 6; }
        d.frame();
        d.grab(app.ColourGradeBackBuffer(), "grade_cdl_again.bin");

        // a strip with the stage on: Draw throws, and the whole frame works again afterwards
        app.SetStrip(0, H / 2);
        d.gt.Tick(1.0f / 60.0f);
        app.Update(d.gt);
        try { app.Draw(d.gt); } catch (const CrychicException& e) { refused += e.Status == CRYCHIC_E_INVALID_ARG; }
        if (refused != 6) { std::fprintf(stderr, "a strip with the colour grade on did not throw\n"); return 7; }
        app.SetWholeFrame();

        // a caller's table, and a file
        if (lut5.size() != 4u * 5u * 5u * 5u) { std::fprintf(stderr, "lut5.bin size\n"); return 2; }
        app.SetColourGradeLut(reinterpret_cast<const uint8_t*>(lut5.data()), 5);
        if (app.ColourGradeSize() != 5u) { std::fprintf(stderr, "SetColourGradeLut\n"); return 8; }
        d.frame();
        d.grab(app.ColourGradeBackBuffer(), "grade_lut5.bin");
        app.LoadColourGradeLut((d.dir + "/look.cube").c_str());
        if (app.ColourGradeSize() != 17u) { std::fprintf(stderr, "LoadColourGradeLut\n"); return 9; }
        d.frame();
        d.grab(app.ColourGradeBackBuffer(), "grade_cube.bin");

        // behind the bloom and in front of the anti-aliasing
        app.SetBloom(true);
        app.SetAntiAliasing(true);
        d.frame();
        d.grab(app.BloomBackBuffer(), "grade_bloom_in.bin");
        d.grab(app.ColourGradeBackBuffer(), "grade_bloom.bin");
        d.grab(app.AntiAliasedBackBuffer(), "grade_bloom_aa.bin");
        app.SetAntiAliasing(false);
        app.SetBloom(false);

        // off again
        app.SetColourGrade(nullptr);
        if (app.ColourGrade() || app.ColourGradeBackBuffer() || app.ColourGradeSize() != 0u) { std::fprintf(stderr, "SetColourGrade(nullptr)\n"); return 10; }
        d.frame();
        d.grab(app.CurrentBackBuffer(), "plain_again.bin");
        std::printf("grade driver ok %ux%u\n", W, H);
        return 0;
    });
}
