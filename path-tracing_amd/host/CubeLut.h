// CubeLut.h -- what the display transform's host side needs beyond the C-ABI (ptx.h "Display transform", docs/NEXT_ROWS.md
// section 22): a reader of .cube 3-D LUT files for ptx_grade_lut, and the white-balance matrix for PtxGradeDesc::colourMatrix.
// Header-only on purpose: RendererHip.cpp uses both, and every build line of a RendererHip host lists its sources by name.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace PathTracing
{

struct CubeLut
{
    uint32_t Size = 0;      // N: the lattice is N x N x N
    std::string Title;
    std::vector<float> Rgb; // N^3 x 3, red fastest: what ptx_grade_lut takes
};

namespace CubeLutDetail
{
constexpr uint32_t MinSize = 2, MaxSize = 65; // PTX_GRADE_LUT_MIN_SIZE, PTX_GRADE_LUT_MAX_SIZE

[[noreturn]] inline void Fail(const std::string &path, size_t line, const std::string &what)
{
    throw std::runtime_error("CubeLut: " + path + ":" + std::to_string(line) + ": " + what);
}

// `count` numbers and nothing else on the rest of the line
inline bool Numbers(const char *s, int count, float *out)
{
    for (int i = 0; i < count; i++)
    {
        char *end = nullptr;
        out[i] = std::strtof(s, &end);
        if (end == s || !std::isfinite(out[i]))
            return false;
        s = end;
    }
    while (*s == ' ' || *s == '\t' || *s == '\r')
        s++;
    return *s == '\0';
}

// One pass over the file.  table == nullptr: validate everything and count the rows; otherwise store them.
inline void Scan(const std::string &path, CubeLut &lut, std::vector<float> *table)
{
    std::ifstream in(path);
    if (!in)
        throw std::runtime_error("CubeLut: cannot open " + path);
    std::string line;
    size_t number = 0, rows = 0, want = 0;
    uint32_t size = 0;
    while (std::getline(in, line))
    {
        number++;
        size_t at = line.find_first_not_of(" \t\r");
        if (at == std::string::npos || line[at] == '#')
            continue;
        const char *s = line.c_str() + at;
        const auto keyword = [&](const char *word) {
            const size_t n = std::char_traits<char>::length(word);
            return line.compare(at, n, word) == 0 && (line.size() == at + n || line[at + n] == ' ' || line[at + n] == '\t');
        };
        float v[3];
        if (keyword("TITLE"))
        {
            const size_t a = line.find('"', at), b = line.rfind('"');
            if (a == std::string::npos || b == a)
                Fail(path, number, "TITLE needs a quoted string");
            lut.Title = line.substr(a + 1, b - a - 1);
        }
        else if (keyword("LUT_3D_SIZE"))
        {
            if (size || !Numbers(s + 11, 1, v) || v[0] != std::floor(v[0]) || v[0] < (float)MinSize || v[0] > (float)MaxSize)
                Fail(path, number, "LUT_3D_SIZE must be given once, an integer in 2 .. 65");
            size = (uint32_t)v[0];
            want = (size_t)size * size * size;
        }
        else if (keyword("DOMAIN_MIN") || keyword("DOMAIN_MAX"))
        {
            const float bound = line[at + 8] == 'I' ? 0.0f : 1.0f; // DOMAIN_MIN / DOMAIN_MAX
            if (!Numbers(s + 10, 3, v) || v[0] != bound || v[1] != bound || v[2] != bound)
                Fail(path, number, "only DOMAIN_MIN 0 0 0 and DOMAIN_MAX 1 1 1 are accepted");
        }
        else if ((*s >= 'A' && *s <= 'Z') || (*s >= 'a' && *s <= 'z') || *s == '_')
            Fail(path, number, "unknown keyword (a 1-D LUT or a shaper is not read)");
        else
        {
            if (!size)
                Fail(path, number, "a table row ahead of LUT_3D_SIZE");
            if (!Numbers(s, 3, v))
                Fail(path, number, "a table row must be three finite numbers");
            if (rows == want)
                Fail(path, number, "more than LUT_3D_SIZE^3 table rows");
            if (table)
            {
                float *row = table->data() + rows * 3;
                row[0] = v[0]; row[1] = v[1]; row[2] = v[2];
            }
            rows++;
        }
    }
    if (!size)
        throw std::runtime_error("CubeLut: " + path + ": no LUT_3D_SIZE");
    if (rows != want)
        throw std::runtime_error("CubeLut: " + path + ": truncated, " + std::to_string(rows) + " table rows of " + std::to_string(want));
    lut.Size = size;
}
} // namespace CubeLutDetail

// Reads a .cube file: LUT_3D_SIZE, DOMAIN_MIN / DOMAIN_MAX (only 0 and 1), TITLE, # comments, N^3 rows of three numbers, red fastest.
// Anything else -- a missing or repeated size, a size outside 2 .. 65, another domain, an unknown keyword, a row that is not three
// finite numbers, too few or too many rows -- throws std::runtime_error.  The file is validated and its rows are counted in a first
// pass; the table is allocated only then, and filled in a second.
inline CubeLut ReadCubeLut(const std::string &path)
{
    CubeLut lut;
    CubeLutDetail::Scan(path, lut, nullptr);
    lut.Rgb.resize((size_t)lut.Size * lut.Size * lut.Size * 3);
    CubeLutDetail::Scan(path, lut, &lut.Rgb);
    return lut;
}

namespace CubeLutDetail
{
struct M3
{
    double m[3][3];
};
inline M3 Mul(const M3 &a, const M3 &b)
{
    M3 r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
    return r;
}
inline M3 Inverse(const M3 &a)
{
    const double(*m)[3] = a.m;
    M3 c;
    c.m[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1]; c.m[0][1] = m[0][2] * m[2][1] - m[0][1] * m[2][2]; c.m[0][2] = m[0][1] * m[1][2] - m[0][2] * m[1][1];
    c.m[1][0] = m[1][2] * m[2][0] - m[1][0] * m[2][2]; c.m[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0]; c.m[1][2] = m[0][2] * m[1][0] - m[0][0] * m[1][2];
    c.m[2][0] = m[1][0] * m[2][1] - m[1][1] * m[2][0]; c.m[2][1] = m[0][1] * m[2][0] - m[0][0] * m[2][1]; c.m[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0];
    const double det = m[0][0] * c.m[0][0] + m[0][1] * c.m[1][0] + m[0][2] * c.m[2][0];
    for (auto &row : c.m)
        for (double &v : row)
            v /= det;
    return c;
}
inline void Apply(const M3 &a, const double v[3], double out[3])
{
    for (int i = 0; i < 3; i++)
        out[i] = a.m[i][0] * v[0] + a.m[i][1] * v[1] + a.m[i][2] * v[2];
}
inline void XyToXyz(double x, double y, double out[3]) // Y = 1
{
    out[0] = x / y; out[1] = 1.0; out[2] = (1.0 - x - y) / y;
}
} // namespace CubeLutDetail

// The matrix, row-major and in linear sRGB, that turns the light of a black body at `kelvin` into white: Krystek's rational
// approximation of the Planckian locus (1985, CIE 1960 u, v; 1000 .. 15000 K) gives the source's chromaticity, a Bradford adaptation
// maps it to the sRGB white (0.3127, 0.3290), and the sRGB primaries (0.64, 0.33), (0.30, 0.60), (0.15, 0.06) with that white express it
// in RGB.  All in float64, rounded once.  kelvin = 0 is the identity matrix: no white balance, and ptx_grade skips the step.
inline void WhiteBalanceMatrix(double kelvin, float out[9])
{
    using namespace CubeLutDetail;
    if (kelvin == 0.0)
    {
        for (int i = 0; i < 9; i++)
            out[i] = i % 4 == 0 ? 1.0f : 0.0f;
        return;
    }
    if (!(kelvin >= 1000.0 && kelvin <= 15000.0))
        throw std::runtime_error("WhiteBalanceMatrix: the temperature must be 0 or within 1000 .. 15000 K");
    const double T = kelvin;
    const double u = (0.860117757 + 1.54118254e-4 * T + 1.28641212e-7 * T * T) / (1.0 + 8.42420235e-4 * T + 7.08145163e-7 * T * T);
    const double v = (0.317398726 + 4.22806245e-5 * T + 4.20481691e-8 * T * T) / (1.0 - 2.89741816e-5 * T + 1.61456053e-7 * T * T);
    const double x = 3.0 * u / (2.0 * u - 8.0 * v + 4.0), y = 2.0 * v / (2.0 * u - 8.0 * v + 4.0);
    double source[3], white[3];
    XyToXyz(x, y, source);
    XyToXyz(0.3127, 0.3290, white);
    // RGB -> XYZ: the primaries' XYZ as columns, scaled so that RGB (1, 1, 1) is the white
    const double prim[3][2] = { { 0.64, 0.33 }, { 0.30, 0.60 }, { 0.15, 0.06 } };
    M3 P;
    for (int k = 0; k < 3; k++)
    {
        double c[3];
        XyToXyz(prim[k][0], prim[k][1], c);
        for (int i = 0; i < 3; i++)
            P.m[i][k] = c[i];
    }
    double scale[3];
    Apply(Inverse(P), white, scale);
    M3 rgbToXyz = P;
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++)
            rgbToXyz.m[i][k] *= scale[k];
    const M3 bradford = { { { 0.8951, 0.2664, -0.1614 }, { -0.7502, 1.7135, 0.0367 }, { 0.0389, -0.0685, 1.0296 } } };
    double coneSource[3], coneWhite[3];
    Apply(bradford, source, coneSource);
    Apply(bradford, white, coneWhite);
    M3 gain = { { { coneWhite[0] / coneSource[0], 0, 0 }, { 0, coneWhite[1] / coneSource[1], 0 }, { 0, 0, coneWhite[2] / coneSource[2] } } };
    const M3 adapt = Mul(Inverse(bradford), Mul(gain, bradford));
    const M3 m = Mul(Inverse(rgbToXyz), Mul(adapt, rgbToXyz));
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            out[3 * i + j] = (float)m.m[i][j];
}

} // namespace PathTracing
