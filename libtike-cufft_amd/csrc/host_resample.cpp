// host_resample.cpp -- the plain-C++ index logic of k_resample.hpp, walked on the CPU (make host_resample):
//   1. the segment / warm-up plan of the prefilter, emulated in float64, against the whole-line exact filter, and the
//      exact filter against the interpolation condition sum_j beta(j) c[refl(k + j)] = x[k];
//   2. the mirror reflection against a walk that bounces between the ends;
//   3. the B-spline weights: partition of unity and the values at the integers;
//   4. the warp's source box: it contains every tap of every pixel the tile evaluates, it fits LDS when it says so, and a
//      tile that claims to lie outside evaluates nothing.
// Prints one line per part and "host_resample: 0 errors"; exits 1 otherwise.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "k_resample.hpp"

using namespace pty;

namespace {

long long errors = 0;

void expect(const bool ok, const char* what, const long long a = 0, const long long b = 0, const long long c = 0) {
    if (ok) return;
    if (++errors <= 20) std::printf("FAIL %s (%lld, %lld, %lld)\n", what, a, b, c);
}

unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
double uniform() {   // xorshift64*, in [-1, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545f4914f6cdd1dull) >> 11) / 4503599627370496.0 - 1.0;
}

const double kBeta[6][5] = {{1.0}, {1.0}, {0.125, 0.75, 0.125}, {1.0 / 6, 4.0 / 6, 1.0 / 6},
                            {1.0 / 384, 76.0 / 384, 230.0 / 384, 76.0 / 384, 1.0 / 384},
                            {1.0 / 120, 26.0 / 120, 66.0 / 120, 26.0 / 120, 1.0 / 120}};

double check_prefilter() {
    double worst = 0.0;
    long long lines = 0;
    for (int order = 2; order <= 5; ++order) {
        double z[2];
        const int np = rs_poles(order, z), halo = rs_halo(order);
        const double gain = rs_gain(order);
        expect(halo % 4 == 0 && halo <= kRsMaxHalo, "halo", order, halo);
        for (int p = 0; p < np; ++p) expect(std::pow(std::fabs(z[p]), halo) <= 1e-9, "warm-up", order, p);
        const int L = kRsSeg;
        const int lens[] = {2, 3, halo, L - 1, L, L + 1, 2 * L + 1, L + halo, L + halo + 1, 4 * L + 3, 7 * L};
        for (const int n : lens) {
            std::vector<double> x(n), exact(n), plan(n), buf;
            for (double& v : x) v = uniform();
            for (int i = 0; i < n; ++i) exact[i] = gain * x[i];
            rs_filter_line<double>(exact.data(), 1, n, true, true, n, z, np);
            double top = 0.0;
            for (const double v : exact) top = std::fmax(top, std::fabs(v));
            const int taps = order / 2;
            for (int k = 0; k < n; ++k) {   // the coefficients interpolate the samples
                double s = 0.0;
                for (int j = -taps; j <= taps; ++j) s += kBeta[order][j + taps] * exact[rs_reflect(k + j, n)];
                expect(std::fabs(s - x[k]) <= 1e-12 * top, "interpolation", order, n, k);
            }
            expect(rs_segments(n) == (n + L - 1) / L, "segments", n);
            int next = 0;
            for (int s = 0; s < rs_segments(n); ++s) {
                const RsSeg g = rs_segment(s, n, halo);
                expect(g.s0 == next && g.s1 > g.s0 && g.s1 <= n && g.a0 >= 0 && g.a0 <= g.s0 && g.b1 >= g.s1 && g.b1 <= n &&
                           g.b1 - g.a0 >= 2 && g.b1 - g.a0 <= L + 2 * halo && g.a0 % 4 == 0,
                       "segment", n, s);
                expect(g.a0 == 0 || g.s0 - g.a0 == halo, "left warm-up", n, s);
                expect(g.b1 == n || g.b1 - g.s1 == halo, "right warm-up", n, s);
                next = g.s1;
                const int len = g.b1 - g.a0;
                buf.assign(len, 0.0);
                for (int i = 0; i < len; ++i) buf[i] = gain * x[g.a0 + i];
                rs_filter_line<double>(buf.data(), 1, len, g.a0 == 0, g.b1 == n, n, z, np);
                for (int i = g.s0; i < g.s1; ++i) plan[i] = buf[i - g.a0];
            }
            expect(next == n, "cover", n);
            for (int i = 0; i < n; ++i) {
                const double e = std::fabs(plan[i] - exact[i]) / top;
                worst = std::fmax(worst, e);
                expect(e <= 1e-8, "plan against the exact filter", order, n, i);
            }
            ++lines;
        }
    }
    std::printf("prefilter: %lld lines, plan within %.2e of the exact filter\n", lines, worst);
    return worst;
}

void check_reflect() {
    long long cases = 0;
    for (int n = 2; n <= 11; ++n) {
        int pos = 0, dir = 1;
        for (int i = 0; i <= 70; ++i) {   // walk right from 0, bouncing
            expect(rs_reflect(i, n) == pos && rs_reflect(-i, n) == pos, "reflect", n, i, pos);
            if (pos + dir < 0 || pos + dir > n - 1) dir = -dir;
            pos += dir;
            cases += 2;
        }
    }
    expect(rs_reflect(1 << 30, 65536) >= 0 && rs_reflect(-(1 << 30), 65536) < 65536, "reflect far");
    std::printf("reflect: %lld cases\n", cases);
}

template <int ORDER>
void check_weights_order() {
    float w[ORDER + 1];
    for (int i = 0; i <= 1000; ++i) {
        const float t = (ORDER & 1) ? (float)i / 1001.0f : (float)i / 1001.0f - 0.5f;
        rs_weights<ORDER>(t, w);
        double s = 0.0;
        for (int a = 0; a <= ORDER; ++a) {
            s += w[a];
            expect(w[a] >= -1e-7f && w[a] <= 1.0f, "weight range", ORDER, i, a);
        }
        expect(std::fabs(s - 1.0) <= 1e-6, "partition of unity", ORDER, i);
    }
    if (ORDER >= 2) {   // t = 0: the values at the integers
        rs_weights<ORDER>(0.0f, w);
        const int taps = ORDER / 2;
        for (int a = 0; a <= ORDER; ++a) {
            const double want = a <= 2 * taps ? kBeta[ORDER][a] : 0.0;
            expect(std::fabs(w[a] - want) <= 1e-6, "weights at an integer", ORDER, a);
        }
    }
}

void check_weights() {
    check_weights_order<0>();
    check_weights_order<1>();
    check_weights_order<2>();
    check_weights_order<3>();
    check_weights_order<4>();
    check_weights_order<5>();
    std::printf("weights: orders 0 .. 5\n");
}

void check_boxes() {
    struct Xf { double m[4], oy, ox; };
    std::vector<Xf> xfs;
    const double pi = 3.14159265358979323846;
    for (const double deg : {0.0, 17.3, 45.0, 90.0, -120.0, 180.0})
        for (const double sc : {1.0, 0.83, 2.5}) {
            const double c = std::cos(deg * pi / 180) * sc, s = std::sin(deg * pi / 180) * sc;
            xfs.push_back({{c, s, -s, c}, 3.2, -1.7});
            xfs.push_back({{c, s, -s, c}, 18.0, 26.0});
        }
    xfs.push_back({{0.5, 0.0, 0.0, 3.0}, 0.0, 0.0});        // anisotropic scales
    xfs.push_back({{5.0, 0.0, 0.0, 5.0}, 0.0, 0.0});        // minification: the global path
    xfs.push_back({{1.0, 0.4, 0.0, 1.0}, -2.0, 1.0});       // shears
    xfs.push_back({{1.0, 0.0, -0.7, 1.2}, 4.0, 9.5});
    xfs.push_back({{1.0, 0.0, 0.0, 1.0}, -40.0, 0.0});      // tiles partly and wholly outside
    xfs.push_back({{1.0, 0.0, 0.0, 1.0}, 0.0, 1000.0});
    xfs.push_back({{1.0, 0.0, 0.0, 1.0}, -1e-7, 1e-7});     // within the clamp
    xfs.push_back({{36.0 / 40.0, 0.0, 0.0, 52.0 / 46.0}, 0.0, 0.0});   // zoom's corner-aligned map
    const int shapes[][4] = {{37, 53, 41, 47}, {300, 300, 60, 60}, {2, 2, 70, 90}, {64, 64, 64, 64}, {5, 200, 33, 65}};
    long long tiles[3] = {0, 0, 0}, pixels = 0;
    for (const auto& sh : shapes)
        for (const Xf& t : xfs)
            for (int order = 0; order <= 5; ++order)
                for (const int flags : {0, (int)RS_MIRROR, (int)RS_GLOBAL}) {
                    const int ny = sh[0], nx = sh[1], oh = sh[2], ow = sh[3];
                    const double xf[6] = {t.m[0], t.m[1], t.m[2], t.m[3], t.oy, t.ox};
                    for (int ty = 0; ty * kRsTile < oh; ++ty)
                        for (int tx = 0; tx * kRsTile < ow; ++tx) {
                            const int oy0 = ty * kRsTile, ox0 = tx * kRsTile;
                            const int oy1 = std::min(oy0 + kRsTile, oh) - 1, ox1 = std::min(ox0 + kRsTile, ow) - 1;
                            const RsBox b = rs_tile_box(xf, oy0, oy1, ox0, ox1, ny, nx, order, flags);
                            ++tiles[b.path];
                            if (b.path != RS_PATH_CVAL)
                                expect(b.y0 >= 0 && b.x0 >= 0 && b.h >= 1 && b.w >= 1 && b.y0 + b.h <= ny && b.x0 + b.w <= nx, "box in image");
                            if (b.path == RS_PATH_LDS) expect((long long)b.h * (b.w | 1) <= kRsBoxElems, "box fits", b.h, b.w);
                            if (flags & RS_GLOBAL) expect(b.path != RS_PATH_LDS, "forced global");
                            for (int oy = oy0; oy <= oy1; ++oy)
                                for (int ox = ox0; ox <= ox1; ++ox) {
                                    double sy = rs_coord(xf[0], xf[1], xf[4], oy, ox), sx = rs_coord(xf[2], xf[3], xf[5], oy, ox);
                                    if (!rs_inside(sy, sx, ny, nx, flags)) continue;
                                    ++pixels;
                                    expect(b.path != RS_PATH_CVAL, "evaluated pixel in a tile that claims to be outside", oy, ox);
                                    if (b.path != RS_PATH_LDS) continue;
                                    float fy, fx;
                                    const int by = rs_first_tap(sy, order, fy), bx = rs_first_tap(sx, order, fx);
                                    expect(fy >= ((order & 1) ? 0.0f : -0.5f) && fy <= ((order & 1) ? 1.0f : 0.5f), "fraction", oy, ox);
                                    for (int a = 0; a <= order; ++a) {
                                        const int iy = rs_reflect(by + a, ny) - b.y0, ix = rs_reflect(bx + a, nx) - b.x0;
                                        expect(iy >= 0 && iy < b.h && ix >= 0 && ix < b.w, "tap outside the box", oy, ox, a);
                                    }
                                }
                        }
                }
    expect(tiles[0] > 0 && tiles[1] > 0 && tiles[2] > 0, "every path is reached", tiles[0], tiles[1], tiles[2]);
    // a 32 x 32 tile under any rotation at unit scale stays on the LDS path
    for (int deg = 0; deg < 360; deg += 5) {
        const double c = std::cos(deg * pi / 180), s = std::sin(deg * pi / 180);
        const double xf[6] = {c, s, -s, c, 1024.0 - 1024.0 * (c + s), 1024.0 - 1024.0 * (c - s)};
        const RsBox b = rs_tile_box(xf, 1024, 1055, 1024, 1055, 2048, 2048, 5, 0);
        expect(b.path == RS_PATH_LDS, "unit-scale rotation on the LDS path", deg, b.h, b.w);
    }
    std::printf("boxes: %lld tiles outside, %lld LDS, %lld global, %lld pixels evaluated\n", tiles[0], tiles[1], tiles[2], pixels);
}

}  // namespace

int main() {
    check_prefilter();
    check_reflect();
    check_weights();
    check_boxes();
    std::printf("host_resample: %lld errors\n", errors);
    return errors ? 1 : 0;
}
