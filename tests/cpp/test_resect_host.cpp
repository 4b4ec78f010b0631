// test_resect_host.cpp -- the host half of batched camera resection (surikatoko_amd/csrc/srk_resect.cpp) without a GPU, driven by
// tests/test_resect_cpu.py.  Built with the host compiler alone:
//   c++ -std=c++17 tests/cpp/test_resect_host.cpp surikatoko_amd/csrc/srk_resect.cpp
// Usage:
//   test_resect_host unit             the argument checks, the option defaults and the coordinate maps; exit status 0 = all hold
//   test_resect_host frames IN OUT    IN: int64 { n_frames, n_obs, n_points, has_q, attempts, loss_kind, want_weights }, double { f0,
//                                     rel_change, loss_delta }, then row_ptr (int64), point (int32), uv, q (if has_q), X, K [n][9],
//                                     R0, T0 as raw arrays.  OUT: R [n][9], T [n][3], quality [n][6], info [n][36] (doubles), status
//                                     [n] (uint32), the attempts logged per frame [n] (int32), the logs (int32: 1 accepted), and
//                                     w_out [n_obs] (if want_weights): every frame walked on the host in the kernel's order of
//                                     operations (srk_resect_host_frame).
#include "../../surikatoko_amd/csrc/srk_resect.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

namespace {
int failures = 0;
void expect(bool ok, const char* what)
{
    if (!ok) {
        std::fprintf(stderr, "FAILED: %s\n", what);
        ++failures;
    }
}
bool refused(const std::string& why, const char* part) { return !why.empty() && why.find(part) != std::string::npos; }

int unit()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    // defaults
    srk_resect_options o;
    std::memset(&o, 0xff, sizeof o);
    srk_resect_default_options(&o);
    expect(o.attempts == 10 && o.rel_change == 1e-9 && o.loss_kind == 0 && o.loss_delta_pixels == 0.0, "default options");
    expect(srk_resect_effective_options(nullptr).attempts == 10, "NULL options = the defaults");
    o.attempts = 7;
    expect(srk_resect_effective_options(&o).attempts == 7, "given options are taken");
    srk_resect_default_options(&o);

    // a good batch: frames of 0, 1 and 3 observations over 4 landmarks
    const int64_t rp[] = { 0, 0, 1, 4 };
    const int32_t pt[] = { 3, 0, 1, 2 };
    const double uv[] = { 1, 2, 3, 4, 5, 6, 7, 8 };
    const double q[] = { 1, 0, 2.5, 1 };
    const double X[] = { 0, 0, 5, 1, 0, 5, 0, 1, 5, 1, 1, 6 };
    const double I3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    double K[27], R0[27], T0[9] = { 0, 0, 0, 0, 0, 1, 0.5, 0, 0 };
    for (int j = 0; j < 3; ++j) std::memcpy(K + 9 * j, I3, sizeof I3), std::memcpy(R0 + 9 * j, I3, sizeof I3);
    auto chk = [&](int32_t n, const int64_t* a, const int32_t* b, const double* c, const double* d, int64_t np, const double* x, const double* k,
                   int shared, const double* r, const double* t, const srk_resect_options* op) {
        return srk_resect_check(n, a, b, c, d, np, x, k, shared, r, t, op);
    };
    expect(chk(3, rp, pt, uv, q, 4, X, K, 0, R0, T0, &o).empty(), "a good batch passes");
    expect(chk(3, rp, pt, uv, nullptr, 4, X, K, 1, R0, T0, nullptr).empty(), "q and options may be NULL, K may be shared");
    expect(chk(0, rp, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr).empty(), "no frames, no arrays");
    // every refusal
    expect(refused(chk(-1, rp, pt, uv, q, 4, X, K, 0, R0, T0, &o), "negative frame count"), "negative count");
    expect(refused(chk(3, nullptr, pt, uv, q, 4, X, K, 0, R0, T0, &o), "row_ptr is NULL"), "NULL row_ptr");
    expect(refused(chk(3, rp, nullptr, uv, q, 4, X, K, 0, R0, T0, &o), "NULL observation array"), "NULL point");
    expect(refused(chk(3, rp, pt, nullptr, q, 4, X, K, 0, R0, T0, &o), "NULL observation array"), "NULL uv");
    expect(refused(chk(3, rp, pt, uv, q, 4, X, nullptr, 0, R0, T0, &o), "NULL pose or intrinsics"), "NULL K");
    expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, nullptr, T0, &o), "NULL pose or intrinsics"), "NULL R0");
    expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, R0, nullptr, &o), "NULL pose or intrinsics"), "NULL T0");
    {
        const char* why = nullptr;
        expect(srk_resect_check_frames(3, rp, pt, uv, q, 4, nullptr, K, 0, R0, T0, &o, &why) == SRK_E_ARGS && std::strstr(why, "landmark array is NULL"),
               "NULL X with a positive count");
        expect(srk_resect_check_frames(3, rp, pt, uv, q, 4, X, K, 0, R0, T0, &o, &why) == SRK_OK && why && !*why, "C entry: fine");
        expect(srk_resect_check_frames(3, rp, pt, uv, q, 3, X, K, 0, R0, T0, &o, nullptr) == SRK_E_ARGS, "C entry: why may be NULL");
    }
    {
        const int64_t bad[] = { 1, 1, 2, 4 }, dec[] = { 0, 2, 1, 4 };
        expect(refused(chk(3, bad, pt, uv, q, 4, X, K, 0, R0, T0, &o), "row_ptr[0]"), "row_ptr starts at 0");
        expect(refused(chk(3, dec, pt, uv, q, 4, X, K, 0, R0, T0, &o), "decreases at frame 1"), "decreasing row_ptr");
    }
    {
        const int32_t hi[] = { 3, 0, 4, 2 }, lo[] = { 3, -1, 1, 2 };
        expect(refused(chk(3, rp, hi, uv, q, 4, X, K, 0, R0, T0, &o), "observation 2 is out of range"), "point == n_points");
        expect(refused(chk(3, rp, lo, uv, q, 4, X, K, 0, R0, T0, &o), "observation 1 is out of range"), "negative point");
    }
    for (double bad : { nan, inf }) {
        double m[8], w[4], x[12], k[27], r[27], t[9];
        std::memcpy(m, uv, sizeof m), std::memcpy(w, q, sizeof w), std::memcpy(x, X, sizeof x), std::memcpy(k, K, sizeof k);
        std::memcpy(r, R0, sizeof r), std::memcpy(t, T0, sizeof t);
        m[5] = bad, w[3] = bad, x[7] = bad, k[13] = bad, r[20] = bad, t[4] = bad;
        expect(refused(chk(3, rp, pt, m, q, 4, X, K, 0, R0, T0, &o), "uv of observation 2"), "uv not finite");
        expect(refused(chk(3, rp, pt, uv, w, 4, X, K, 0, R0, T0, &o), "q of observation 3"), "q not finite");
        expect(refused(chk(3, rp, pt, uv, q, 4, x, K, 0, R0, T0, &o), "landmark 2 is not finite"), "X not finite");
        expect(refused(chk(3, rp, pt, uv, q, 4, X, k, 0, R0, T0, &o), "K of frame 1 is not finite"), "K not finite");
        expect(chk(3, rp, pt, uv, q, 4, X, k, 1, R0, T0, &o).empty(), "a shared K is one matrix");
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, r, T0, &o), "R0 of frame 2 is not finite"), "R0 not finite");
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, R0, t, &o), "T0 of frame 1 is not finite"), "T0 not finite");
    }
    {
        double w[4], r[27];
        std::memcpy(w, q, sizeof w), std::memcpy(r, R0, sizeof r);
        w[3] = -1e-300;
        expect(refused(chk(3, rp, pt, uv, w, 4, X, K, 0, R0, T0, &o), "q of observation 3"), "negative q");
        r[9] = 1.0 + 1e-8;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, r, T0, &o), "R0 of frame 1 is not orthogonal to 1e-9"), "scaled rotation");
        r[9] = 1.0 + 1e-11;
        expect(chk(3, rp, pt, uv, q, 4, X, K, 0, r, T0, &o).empty(), "a rotation to 1e-9 passes");
        r[9] = -1.0;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, r, T0, &o), "determinant"), "a reflection");
    }
    {
        srk_resect_options b = o;
        b.attempts = SRK_RESECT_MAX_ATTEMPTS_HOST + 1;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, R0, T0, &b), "attempts"), "too many attempts");
        b.attempts = SRK_RESECT_MAX_ATTEMPTS_HOST;
        expect(chk(3, rp, pt, uv, q, 4, X, K, 0, R0, T0, &b).empty(), "64 attempts are allowed");
        b.attempts = -1;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, R0, T0, &b), "attempts"), "negative attempts");
        b = o, b.rel_change = -1;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, R0, T0, &b), "rel_change"), "negative rel change");
        b = o, b.rel_change = nan;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, R0, T0, &b), "rel_change"), "NaN rel change");
        b = o, b.loss_kind = 3;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, R0, T0, &b), "loss_kind"), "unknown loss");
        b = o, b.loss_kind = -1;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, R0, T0, &b), "loss_kind"), "negative loss kind");
        b = o, b.loss_kind = 1;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, R0, T0, &b), "loss_delta_pixels"), "a loss without delta");
        b.loss_delta_pixels = 2.0;
        expect(chk(3, rp, pt, uv, q, 4, X, K, 0, R0, T0, &b).empty(), "Huber at 2 px");
    }
    // the landmark order, applied inside the check loop
    {
        const int64_t to_int[] = { 2, 3, 0, 1 };
        std::vector<int32_t> out;
        expect(chk(3, rp, pt, uv, q, 4, nullptr, K, 0, R0, T0, &o).empty(), "X may be NULL for the resident scene");
        expect(srk_resect_check(3, rp, pt, uv, q, 4, nullptr, K, 0, R0, T0, &o, to_int, &out).empty() && out.size() == 4 && out[0] == 1 && out[1] == 2 &&
                   out[2] == 3 && out[3] == 0,
               "points through the order");
        expect(srk_resect_check(3, rp, pt, uv, q, 4, nullptr, K, 0, R0, T0, &o, nullptr, &out).empty() && out[0] == 3 && out[3] == 2, "no order = the same points");
    }
    // the map into the normalised coordinates and back: X_n = s (R0 X + T0) keeps x_cam up to the scale
    {
        srk_ba_normalizer nrm;
        const double c = std::cos(0.3), s = std::sin(0.3);
        const double N0[9] = { c, -s, 0, s, c, 0, 0, 0, 1 };
        std::memcpy(nrm.R0, N0, sizeof N0);
        nrm.T0[0] = 0.5, nrm.T0[1] = -2, nrm.T0[2] = 3;
        nrm.world_scale = 2.5;
        const double c2 = std::cos(-0.7), s2 = std::sin(-0.7);
        const double R[18] = { 1, 0, 0, 0, c2, -s2, 0, s2, c2, c2, 0, s2, 0, 1, 0, -s2, 0, c2 };
        const double T[6] = { 0.25, -1.5, 2, -3, 0.5, 0.125 };
        double Rn[18], Tn[6], info[72], keep[72];
        srk_resect_normalize_poses(nrm, 2, R, T, Rn, Tn);
        const double Xw[3] = { 1.25, -0.75, 4 };
        double Xn[3];
        for (int a = 0; a < 3; ++a) Xn[a] = nrm.world_scale * (N0[3 * a] * Xw[0] + N0[3 * a + 1] * Xw[1] + N0[3 * a + 2] * Xw[2] + nrm.T0[a]);
        for (int j = 0; j < 2; ++j)
            for (int a = 0; a < 3; ++a) {
                const double cam = R[9 * j + 3 * a] * Xw[0] + R[9 * j + 3 * a + 1] * Xw[1] + R[9 * j + 3 * a + 2] * Xw[2] + T[3 * j + a];
                const double camn = Rn[9 * j + 3 * a] * Xn[0] + Rn[9 * j + 3 * a + 1] * Xn[1] + Rn[9 * j + 3 * a + 2] * Xn[2] + Tn[3 * j + a];
                expect(std::fabs(camn - nrm.world_scale * cam) < 1e-13, "the normalised pose sees the normalised point at s x_cam");
            }
        for (int e = 0; e < 72; ++e) { // two symmetric matrices
            const int r = (e % 36) / 6, cc = e % 6;
            keep[e] = info[e] = 1.0 + (r == cc ? 10.0 : 0.0) + 0.1 * (r + cc) + 0.01 * r * cc + (e >= 36 ? 0.5 : 0.0);
        }
        expect(srk_resect_revert(&nrm, 2, Rn, Tn, info) == SRK_OK, "revert runs");
        for (int e = 0; e < 18; ++e) expect(std::fabs(Rn[e] - R[e]) < 1e-14, "revert(normalise(R)) = R");
        for (int e = 0; e < 6; ++e) expect(std::fabs(Tn[e] - T[e]) < 1e-14, "revert(normalise(T)) = T");
        // info: D^T L D with D = diag(s R0, R0); carried back by D^-1 = diag(R0^T / s, R0^T), that is by the normaliser of the inverse map
        srk_ba_normalizer inv;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) inv.R0[3 * a + b] = N0[3 * b + a];
        inv.world_scale = 1.0 / nrm.world_scale;
        inv.T0[0] = inv.T0[1] = inv.T0[2] = 0.0;
        double back[72];
        std::memcpy(back, info, sizeof back);
        expect(srk_resect_revert(&inv, 2, nullptr, nullptr, back) == SRK_OK, "revert of info alone");
        double big = 0, diff = 0, moved = 0;
        for (int e = 0; e < 72; ++e) {
            big = std::fmax(big, std::fabs(keep[e]));
            diff = std::fmax(diff, std::fabs(back[e] - keep[e]));
            moved = std::fmax(moved, std::fabs(info[e] - keep[e]));
        }
        expect(diff < 1e-13 * big && moved > 0.1, "info is carried through the round trip");
        for (int r = 0; r < 6; ++r)
            for (int cc = 0; cc < 6; ++cc) expect(info[6 * r + cc] == info[6 * cc + r], "the mapped info is symmetric");
        // the energy is invariant: x^T L x = x_n^T L_n x_n with x_n = D x
        const double x[6] = { 0.1, -0.2, 0.3, 0.01, 0.02, -0.03 };
        double xn[6];
        for (int a = 0; a < 3; ++a) {
            xn[a] = nrm.world_scale * (N0[3 * a] * x[0] + N0[3 * a + 1] * x[1] + N0[3 * a + 2] * x[2]);
            xn[3 + a] = N0[3 * a] * x[3] + N0[3 * a + 1] * x[4] + N0[3 * a + 2] * x[5];
        }
        double e0 = 0, e1 = 0;
        for (int r = 0; r < 6; ++r)
            for (int cc = 0; cc < 6; ++cc) e0 += x[r] * info[6 * r + cc] * x[cc], e1 += xn[r] * keep[6 * r + cc] * xn[cc];
        expect(std::fabs(e0 - e1) < 1e-13 * std::fabs(e1), "the prior's energy is invariant");
        expect(srk_resect_revert(nullptr, 1, Rn, Tn, info) == SRK_E_ARGS && srk_resect_revert(&nrm, 1, Rn, nullptr, info) == SRK_E_ARGS, "revert: bad arguments");
        expect(srk_resect_revert(&nrm, 0, nullptr, nullptr, nullptr) == SRK_OK, "revert: nothing to do");
    }
    // a walk: a frame of two observations is FEW_POINTS and keeps its pose bit for bit
    {
        double R[9], T[3], ql[6], inf[36], w[3];
        const double t0[3] = { 0.1, -0.2, 0.3 };
        const uint32_t st = srk_resect_host_frame(3, pt + 1, uv + 2, q + 1, X, K, R0, t0, 600.0, o, R, T, ql, inf, w);
        expect(st == SRK_RESECT_FEW_POINTS && ql[1] == 2.0 && std::isnan(ql[3]) && ql[5] == 0.0, "two weighted observations: FEW_POINTS");
        expect(std::memcmp(R, R0, sizeof R) == 0 && std::memcmp(T, t0, sizeof T) == 0, "the pose is the start bit for bit");
        expect(w[0] == 0.0 && w[1] == 1.0 && w[2] == 1.0, "w_out: 0 where q = 0, 1 without a loss");
    }
    if (failures == 0) std::printf("ok\n");
    return failures == 0 ? 0 : 1;
}

template <typename T> bool rd(std::FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T> bool wr(std::FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int frames(const char* in, const char* out)
{
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    std::vector<int64_t> hd, rp;
    std::vector<double> par, uv, q, X, K, R0, T0;
    std::vector<int32_t> pt;
    bool ok = rd(f, hd, 7) && rd(f, par, 3);
    const size_t n = ok ? (size_t)hd[0] : 0, O = ok ? (size_t)hd[1] : 0, N = ok ? (size_t)hd[2] : 0;
    ok = ok && rd(f, rp, n + 1) && rd(f, pt, O) && rd(f, uv, 2 * O) && rd(f, q, hd[3] ? O : 0) && rd(f, X, 3 * N) && rd(f, K, 9 * n) && rd(f, R0, 9 * n) &&
         rd(f, T0, 3 * n);
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short file\n"); return 2; }
    srk_resect_options o;
    o.attempts = (int32_t)hd[4];
    o.rel_change = par[1];
    o.loss_kind = (int32_t)hd[5];
    o.loss_delta_pixels = par[2];
    const double* qp = hd[3] ? q.data() : nullptr;
    const std::string why = srk_resect_check((int32_t)n, rp.data(), pt.data(), uv.data(), qp, (int64_t)N, X.data(), K.data(), 0, R0.data(), T0.data(), &o);
    if (!why.empty()) { std::fprintf(stderr, "refused: %s\n", why.c_str()); return 3; }
    std::vector<double> R(9 * n), T(3 * n), ql(6 * n), info(36 * n), w(hd[6] ? O : 0);
    std::vector<uint32_t> st(n);
    std::vector<int32_t> counts(n), logs;
    for (size_t i = 0; i < n; ++i) {
        const int64_t o0 = rp[i];
        std::vector<int> log;
        st[i] = srk_resect_host_frame(rp[i + 1] - o0, pt.data() + o0, uv.data() + 2 * o0, qp ? qp + o0 : nullptr, X.data(), &K[9 * i], &R0[9 * i], &T0[3 * i],
                                      par[0], o, &R[9 * i], &T[3 * i], &ql[6 * i], &info[36 * i], hd[6] ? w.data() + o0 : nullptr, &log);
        counts[i] = (int32_t)log.size();
        logs.insert(logs.end(), log.begin(), log.end());
    }
    std::FILE* g = std::fopen(out, "wb");
    if (!g) return 2;
    ok = wr(g, R) && wr(g, T) && wr(g, ql) && wr(g, info) && wr(g, st) && wr(g, counts) && wr(g, logs) && wr(g, w);
    std::fclose(g);
    return ok ? 0 : 2;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && std::string(argv[1]) == "unit") return unit();
    if (argc == 4 && std::string(argv[1]) == "frames") return frames(argv[2], argv[3]);
    std::fprintf(stderr, "usage: test_resect_host unit | frames IN OUT\n");
    return 2;
}
