// Host-side check of adjreg_map.hpp: emulates the cooperating threads of ONE workgroup of k_cols_adjreg -- T tile with its
// zero border, the accumulators acc[] of every thread, retire (staged and by the owners) -- over runs of positions, and compares every object pixel
// with a direct four-tap scatter in float64.  It also checks that no pixel is retired by a slide of the window while a
// later position of the same window still touches it.  Built by tests/test_adjreg_cpu.py with clang++ (no GPU involved).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "fft_core.hpp"
#include "adjreg_map.hpp"

using namespace pty;

struct PosH { int t, sy, sx; float fy, fx; bool valid; };

template <int N, int NT>
struct Emu {
    using W = AdjRegCfg<N, NT>;
    static constexpr int C = W::C, WC = W::WC, G = W::G, RPG = W::RPG;
    int ntheta, nz, n, nprb, pad;
    std::vector<double> ref, got;   // [ntheta][nz][n][2]
    std::vector<int> slid;          // window lifetime in which a slide retired the pixel
    std::vector<c32> tile;
    std::vector<c32> acc;           // [NT][RPG]
    std::vector<c32> stage;
    int life = 0;
    long long bad_touch = 0, retired_px = 0, slides = 0, staged = 0, anchors = 0;
    std::mt19937 rng{12345};

    Emu(int ntheta_, int nz_, int n_, int nprb_)
        : ntheta(ntheta_), nz(nz_), n(n_), nprb(nprb_), pad((N - nprb_) / 2),
          ref((size_t)ntheta_ * nz_ * n_ * 2, 0.0), got(ref.size(), 0.0), slid((size_t)ntheta_ * nz_ * n_, -1),
          tile(W::TILE, c32{0.f, 0.f}), acc((size_t)NT * RPG, c32{0.f, 0.f}), stage(W::STAGE, c32{0.f, 0.f}) {}

    size_t px(int t, int Y, int X) const { return ((size_t)t * nz + Y) * n + X; }

    // a slide by at most SG groups: the owners move their rows to the stage, then all threads add the staged rows
    void retire_staged(const AdjRegWin& w, int nret) {
        for (int tid = 0; tid < NT; ++tid) {
            const int cw = tid % WC, g = tid / WC;
            if (g >= G) continue;
            const int rank = adjreg_rank<W>(w, g);
            if (rank >= nret) continue;
            for (int r = 0; r < RPG; ++r) {
                stage[adjreg_stage_slot<W>(rank, r, cw)] = acc[(size_t)tid * RPG + r];
                acc[(size_t)tid * RPG + r] = c32{0.f, 0.f};
            }
        }
        for (int o = 0; o < nret * RPG * WC; ++o) {
            const c32 v = stage[o];
            const int Y = w.Ybase + o / WC, X = w.X0 + o % WC;
            if (X >= 0 && X < n && Y < nz) {
                slid[px(w.t, Y, X)] = life;
                if (v.x != 0.0f || v.y != 0.0f) {
                    got[2 * px(w.t, Y, X)] += v.x;
                    got[2 * px(w.t, Y, X) + 1] += v.y;
                    ++retired_px;
                }
            }
        }
    }

    void retire(const AdjRegWin& w, int nret) {
        if (w.t < 0) return;
        for (int tid = 0; tid < NT; ++tid) {
            const int cw = tid % WC, g = tid / WC;
            if (g >= G || adjreg_rank<W>(w, g) >= nret) continue;
            const int Y0 = adjreg_row0<W>(w, g), X = w.X0 + cw;
            for (int r = 0; r < RPG; ++r) {
                c32& v = acc[(size_t)tid * RPG + r];
                const int Y = Y0 + r;
                if (X >= 0 && X < n && Y < nz) {
                    if (nret < G) slid[px(w.t, Y, X)] = life;
                    if (v.x != 0.0f || v.y != 0.0f) {
                        got[2 * px(w.t, Y, X)] += v.x;
                        got[2 * px(w.t, Y, X) + 1] += v.y;
                        ++retired_px;
                    }
                }
                v = c32{0.f, 0.f};
            }
        }
    }

    // one workgroup: strip x0 / C over the run
    void run(const std::vector<PosH>& pos, int x0) {
        AdjRegWin w{-1, 0, 0, 0};
        std::uniform_real_distribution<float> U(-1.0f, 1.0f);
        for (const PosH& q : pos) {
            if (!q.valid) continue;
            // T tile of this position: random on the probe, zero on the padding (the kernel's probe strip is zero there)
            for (int i = 0; i < N; ++i)
                for (int c = 0; c < C; ++c) {
                    const int iy = i - pad, ix = x0 + c - pad;
                    const bool ok = iy >= 0 && iy < nprb && ix >= 0 && ix < nprb;
                    tile[(size_t)(i + 1) * W::P + c + W::COL0] = ok ? c32{U(rng), U(rng)} : c32{0.f, 0.f};
                }
            const int Xa = q.sx + x0 - pad;
            // reference: kernels.cu:73-80 as a scatter, float64
            const double w00 = (1.0 - q.fx) * (1.0 - q.fy), w01 = (double)q.fx * (1.0 - q.fy);
            const double w10 = (1.0 - q.fx) * (double)q.fy, w11 = (double)q.fx * q.fy;
            for (int y = 0; y < nprb; ++y)
                for (int c = 0; c < C; ++c) {
                    const c32 tv = tile[(size_t)(y + pad + 1) * W::P + c + W::COL0];
                    const double wt[4] = {w00, w01, w10, w11};
                    for (int tap = 0; tap < 4; ++tap) {
                        const int Y = q.sy + y + (tap >> 1), X = Xa + c + (tap & 1);
                        if (Y < 0 || Y >= nz || X < 0 || X >= n) continue;
                        ref[2 * px(q.t, Y, X)] += tv.x * wt[tap];
                        ref[2 * px(q.t, Y, X) + 1] += tv.y * wt[tap];
                    }
                }
            const int nret = adjreg_retire_count<W>(w, q.t, Xa, q.sy);
            if (nret > 0) {
                if (nret <= W::SG) { retire_staged(w, nret); ++staged; } else retire(w, nret);
                if (nret >= G) { ++life; ++anchors; } else ++slides;
                adjreg_advance<W>(w, nret, q.t, q.sx, q.sy, x0 - pad);
            }
            // the position must lie inside the live window
            if (q.sy < w.Ybase || q.sy - w.Ybase >= RPG || q.sy + nprb >= w.Ybase + W::HW || Xa < w.X0 || Xa + C >= w.X0 + WC || w.t != q.t) {
                std::printf("window does not hold the position\n");
                std::exit(1);
            }
            // pixels this position touches must not have been retired by a slide of this window
            for (int Y = q.sy; Y <= q.sy + nprb && Y < nz; ++Y)
                for (int X = Xa; X <= Xa + C; ++X)
                    if (X >= 0 && X < n && slid[px(q.t, Y, X)] == life) ++bad_touch;
            for (int tid = 0; tid < NT; ++tid) {
                const int cw = tid % WC, g = tid / WC;
                if (g < G) adjreg_combine<W>(&acc[(size_t)tid * RPG], tile.data(), w, g, cw, Xa, q.sy, pad, q.fy, q.fx);
            }
        }
        retire(w, G);
        ++life;
    }

    double worst() const {
        double err = 0, nrm = 0;
        for (size_t i = 0; i < ref.size(); ++i) {
            err = std::fmax(err, std::fabs(ref[i] - got[i]));
            nrm = std::fmax(nrm, std::fabs(ref[i]));
        }
        return nrm > 0 ? err / nrm : 1.0;
    }
};

template <int N, int NT>
static bool check(int nprb) {
    using E = Emu<N, NT>;
    constexpr int RPG = E::RPG, HW = E::W::HW;
    const int ntheta = 2, nz = 1200, n = N + 120;
    E emu(ntheta, nz, n, nprb);
    std::mt19937 rng(777 + N + nprb);
    auto ri = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    auto frac = [&]() { return (rng() % 5 == 0) ? 0.0f : (float)(rng() % 1000) / 1000.0f; };
    const int steps[10] = {0, 1, RPG - 1, RPG, RPG + 1, 2 * RPG, HW - 1, HW, HW + 1, 3 * HW};
    const int sy_max = nz - nprb / 2, sx_max = n - nprb / 2;   // positions hang over the bottom and the right edge
    int nruns = 0;
    long long npos = 0;
    // (a) one run per row step, all four column offsets inside the bucket
    for (int s = 0; s < 10; ++s) {
        std::vector<PosH> run;
        int sy = 0;
        const int sx0 = 4 * ri(0, 20);
        for (int k = 0; k < 40; ++k) {
            run.push_back(PosH{0, sy, sx0 + k % 4, frac(), frac(), true});
            sy += steps[s];
            if (sy > sy_max) sy = sy_max;
        }
        emu.run(run, 16 * ri(0, N / 16 - 1));
        ++nruns; npos += 40;
    }
    // (b) every run length, random steps from the set, bucket / angle changes, decreasing rows, skipped positions, edges
    for (int len = 1; len <= 128; ++len) {
        std::vector<PosH> run;
        int t = ri(0, 1), sy = ri(0, 3) == 0 ? 0 : ri(0, sy_max), sx = ri(0, 3) == 0 ? sx_max - ri(0, 7) : ri(0, sx_max);
        for (int k = 0; k < len; ++k) {
            const int ev = ri(0, 99);
            if (ev < 5) sx = ri(0, sx_max);                       // bucket change
            else if (ev < 8 && t + 1 < ntheta) { ++t; sy = ri(0, 50); }   // angle change
            else if (ev < 13) { sy -= ri(1, 2 * RPG); if (sy < 0) sy = 0; }   // decreasing row
            else sx = (sx / 4) * 4 + ri(0, 3);                    // same bucket, any offset
            if (sx > sx_max) sx = sx_max;
            run.push_back(PosH{t, sy, sx, frac(), frac(), ev < 93});   // ev >= 93: skipped
            sy += (ri(0, 2) == 0) ? steps[ri(0, 9)] : ri(0, 12);
            if (sy > sy_max) sy = ri(0, 1) ? sy_max : ri(0, 40);
        }
        emu.run(run, 16 * ri(0, N / 16 - 1));
        ++nruns; npos += len;
    }
    const double e = emu.worst();
    const bool ok = e < 1e-5 && emu.bad_touch == 0 && emu.slides > emu.staged && emu.staged > 0 && emu.anchors > 0;
    std::printf("N=%d nprb=%d G=%d RPG=%d HW=%d runs=%d positions=%lld slides=%lld (staged %lld) anchors=%lld retired=%lld touched_after_retire=%lld rel_err=%.3e %s\n",
                N, nprb, E::G, RPG, HW, nruns, npos, emu.slides, emu.staged, emu.anchors, emu.retired_px, emu.bad_touch, e, ok ? "ok" : "BAD");
    return ok;
}

int main() {
    bool ok = true;
    ok = check<256, 256>(256) && ok;
    ok = check<256, 256>(200) && ok;
    ok = check<512, 512>(512) && ok;
    ok = check<512, 512>(300) && ok;
    std::printf("%s\n", ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}
