// test_tri_host.cpp -- the host half of batched triangulation (surikatoko_amd/csrc/srk_tri.cpp) without a GPU, driven by
// tests/test_triangulate_cpu.py.  Built with the host compiler alone:
//   c++ -std=c++17 tests/cpp/test_tri_host.cpp surikatoko_amd/csrc/srk_tri.cpp
// Usage:
//   test_tri_host unit             the argument checks, the option defaults and the coordinate map; exit status 0 = all hold
//   test_tri_host tracks IN OUT    IN: int64 { n_tracks, n_obs, n_frames, has_q, shared_k, refine_attempts }, double { f0,
//                                  refine_rel_change, min_parallax_deg }, then row_ptr (int64), frame (int32), uv, q (if has_q),
//                                  cam_R, cam_T, K as raw arrays.  OUT: X [n][3], quality [n][4] (doubles), status [n] (uint32):
//                                  every track walked on the host in the kernel's order of operations (srk_tri_host_track).
#include "../../surikatoko_amd/csrc/srk_tri.hpp"

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
    // defaults
    srk_tri_options o;
    std::memset(&o, 0xff, sizeof o);
    srk_tri_default_options(&o);
    expect(o.refine_attempts == 10 && o.refine_rel_change == 1e-9 && o.min_parallax_deg == 0.0, "default options");
    const srk_tri_options lin = srk_tri_effective_options(nullptr);
    expect(lin.refine_attempts == 0 && lin.min_parallax_deg == 0.0, "NULL options = linear only");
    expect(srk_tri_effective_options(&o).refine_attempts == 10, "given options are taken");

    // a good batch: tracks of 0, 1 and 3 observations over 4 frames
    const int64_t rp[] = { 0, 0, 1, 4 };
    const int32_t fr[] = { 3, 0, 1, 2 };
    const double uv[] = { 1, 2, 3, 4, 5, 6, 7, 8 };
    const double q[] = { 1, 0, 2.5, 1 };
    expect(srk_tri_check(3, rp, fr, uv, q, 4, &o).empty(), "a good batch passes");
    expect(srk_tri_check(3, rp, fr, uv, nullptr, 4, nullptr).empty(), "q and options may be NULL");
    expect(srk_tri_check(0, rp, nullptr, nullptr, nullptr, 1, nullptr).empty(), "no tracks, no arrays");
    // every refusal
    expect(refused(srk_tri_check(-1, rp, fr, uv, q, 4, &o), "negative track count"), "negative count");
    expect(refused(srk_tri_check(3, nullptr, fr, uv, q, 4, &o), "row_ptr is NULL"), "NULL row_ptr");
    expect(refused(srk_tri_check(3, rp, nullptr, uv, q, 4, &o), "NULL observation array"), "NULL frame");
    expect(refused(srk_tri_check(3, rp, fr, nullptr, q, 4, &o), "NULL observation array"), "NULL uv");
    expect(refused(srk_tri_check(3, rp, fr, uv, q, 0, &o), "at least one frame"), "no frames");
    {
        const int64_t bad[] = { 1, 1, 2, 4 };
        expect(refused(srk_tri_check(3, bad, fr, uv, q, 4, &o), "row_ptr[0]"), "row_ptr starts at 0");
        const int64_t dec[] = { 0, 2, 1, 4 };
        expect(refused(srk_tri_check(3, dec, fr, uv, q, 4, &o), "decreases at track 1"), "decreasing row_ptr");
    }
    {
        const int32_t hi[] = { 3, 0, 4, 2 }, lo[] = { 3, -1, 1, 2 };
        expect(refused(srk_tri_check(3, rp, hi, uv, q, 4, &o), "observation 2 is out of range"), "frame == n_frames");
        expect(refused(srk_tri_check(3, rp, lo, uv, q, 4, &o), "observation 1 is out of range"), "negative frame");
    }
    {
        double m[8];
        std::memcpy(m, uv, sizeof m);
        m[5] = std::numeric_limits<double>::quiet_NaN();
        expect(refused(srk_tri_check(3, rp, fr, m, q, 4, &o), "uv of observation 2"), "NaN in uv");
        m[5] = std::numeric_limits<double>::infinity();
        expect(refused(srk_tri_check(3, rp, fr, m, q, 4, &o), "uv of observation 2"), "inf in uv");
    }
    {
        double w[4];
        std::memcpy(w, q, sizeof w);
        w[3] = -1e-300;
        expect(refused(srk_tri_check(3, rp, fr, uv, w, 4, &o), "q of observation 3"), "negative q");
        w[3] = std::numeric_limits<double>::quiet_NaN();
        expect(refused(srk_tri_check(3, rp, fr, uv, w, 4, &o), "q of observation 3"), "NaN q");
        w[3] = std::numeric_limits<double>::infinity();
        expect(refused(srk_tri_check(3, rp, fr, uv, w, 4, &o), "q of observation 3"), "inf q");
    }
    {
        srk_tri_options b = o;
        b.refine_attempts = SRK_TRI_MAX_REFINE_ATTEMPTS_HOST + 1;
        expect(refused(srk_tri_check(3, rp, fr, uv, q, 4, &b), "refine_attempts"), "too many attempts");
        b.refine_attempts = SRK_TRI_MAX_REFINE_ATTEMPTS_HOST;
        expect(srk_tri_check(3, rp, fr, uv, q, 4, &b).empty(), "64 attempts are allowed");
        b.refine_attempts = -1;
        expect(refused(srk_tri_check(3, rp, fr, uv, q, 4, &b), "refine_attempts"), "negative attempts");
        b = o;
        b.refine_rel_change = -1;
        expect(refused(srk_tri_check(3, rp, fr, uv, q, 4, &b), "refine_rel_change"), "negative rel change");
        b = o;
        b.min_parallax_deg = std::numeric_limits<double>::quiet_NaN();
        expect(refused(srk_tri_check(3, rp, fr, uv, q, 4, &b), "min_parallax_deg"), "NaN parallax gate");
    }
    {
        const char* why = nullptr;
        expect(srk_tri_check_tracks(3, rp, fr, uv, q, 4, &o, &why) == SRK_OK && why && !*why, "C entry: fine");
        const int32_t hi[] = { 3, 0, 4, 2 };
        expect(srk_tri_check_tracks(3, rp, hi, uv, q, 4, &o, &why) == SRK_E_ARGS && why && std::strstr(why, "out of range"), "C entry: refusal");
        expect(srk_tri_check_tracks(3, rp, hi, uv, q, 4, &o, nullptr) == SRK_E_ARGS, "C entry: why may be NULL");
    }
    // the frame order
    {
        const int32_t to_int[] = { 2, 3, 0, 1 };
        std::vector<int32_t> out;
        srk_tri_map_frames(4, fr, to_int, out);
        expect(out.size() == 4 && out[0] == 1 && out[1] == 2 && out[2] == 3 && out[3] == 0, "frames through the order");
        srk_tri_map_frames(4, fr, nullptr, out);
        expect(out[0] == 3 && out[3] == 2, "no order = the same frames");
    }
    // the coordinate map is the point map of the scene normalisation, inverted: X_n = s (R0 X + T0)
    {
        srk_ba_normalizer nrm;
        const double c = std::cos(0.3), s = std::sin(0.3);
        const double R0[9] = { c, -s, 0, s, c, 0, 0, 0, 1 };
        std::memcpy(nrm.R0, R0, sizeof R0);
        nrm.T0[0] = 0.5;
        nrm.T0[1] = -2;
        nrm.T0[2] = 3;
        nrm.world_scale = 2.5;
        const double X[3] = { 1.25, -0.75, 4 };
        double Xn[6];
        for (int a = 0; a < 3; ++a) Xn[a] = nrm.world_scale * (R0[3 * a] * X[0] + R0[3 * a + 1] * X[1] + R0[3 * a + 2] * X[2] + nrm.T0[a]);
        Xn[3] = Xn[4] = Xn[5] = std::numeric_limits<double>::quiet_NaN();
        expect(srk_tri_revert_points(&nrm, 2, Xn) == SRK_OK, "revert runs");
        for (int a = 0; a < 3; ++a) expect(std::fabs(Xn[a] - X[a]) < 1e-14, "revert inverts the normalisation");
        expect(std::isnan(Xn[3]) && std::isnan(Xn[4]) && std::isnan(Xn[5]), "NaN stays NaN");
        expect(srk_tri_revert_points(nullptr, 1, Xn) == SRK_E_ARGS && srk_tri_revert_points(&nrm, 1, nullptr) == SRK_E_ARGS, "revert: bad arguments");
        expect(srk_tri_revert_points(&nrm, 0, nullptr) == SRK_OK, "revert: nothing to do");
    }
    if (failures == 0) std::printf("ok\n");
    return failures == 0 ? 0 : 1;
}

template <typename T> bool rd(std::FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int tracks(const char* in, const char* out)
{
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    std::vector<int64_t> hd, rp;
    std::vector<double> par, uv, q, R, T, K;
    std::vector<int32_t> fr;
    bool ok = rd(f, hd, 6) && rd(f, par, 3);
    const size_t n = ok ? (size_t)hd[0] : 0, O = ok ? (size_t)hd[1] : 0, M = ok ? (size_t)hd[2] : 0;
    ok = ok && rd(f, rp, n + 1) && rd(f, fr, O) && rd(f, uv, 2 * O) && rd(f, q, hd[3] ? O : 0) && rd(f, R, 9 * M) && rd(f, T, 3 * M) &&
         rd(f, K, hd[4] ? 9 : 9 * M);
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "short file\n"); return 2; }
    srk_tri_options o;
    o.refine_attempts = (int32_t)hd[5];
    o.refine_rel_change = par[1];
    o.min_parallax_deg = par[2];
    const std::string why = srk_tri_check((int64_t)n, rp.data(), fr.data(), uv.data(), hd[3] ? q.data() : nullptr, (int32_t)M, &o);
    if (!why.empty()) { std::fprintf(stderr, "refused: %s\n", why.c_str()); return 3; }
    std::vector<double> pack;
    srk_tri_host_pack((int32_t)M, R.data(), T.data(), K.data(), (int)hd[4], pack);
    std::vector<double> X(3 * n), ql(4 * n);
    std::vector<uint32_t> st(n);
    for (size_t t = 0; t < n; ++t) {
        const int64_t o0 = rp[t];
        st[t] = srk_tri_host_track(rp[t + 1] - o0, fr.data() + o0, uv.data() + 2 * o0, hd[3] ? q.data() + o0 : nullptr, pack.data(), par[0], o,
                                   &X[3 * t], &ql[4 * t]);
    }
    std::FILE* g = std::fopen(out, "wb");
    if (!g) return 2;
    ok = (n == 0) || (std::fwrite(X.data(), 8, 3 * n, g) == 3 * n && std::fwrite(ql.data(), 8, 4 * n, g) == 4 * n && std::fwrite(st.data(), 4, n, g) == n);
    std::fclose(g);
    return ok ? 0 : 2;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && std::string(argv[1]) == "unit") return unit();
    if (argc == 4 && std::string(argv[1]) == "tracks") return tracks(argv[2], argv[3]);
    std::fprintf(stderr, "usage: test_tri_host unit | tracks IN OUT\n");
    return 2;
}
