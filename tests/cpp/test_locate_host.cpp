// test_locate_host.cpp -- the host half of resection without a start pose (surikatoko_amd/csrc/srk_locate.cpp) without a GPU, driven
// by tests/test_locate_cpu.py.  Built with the host compiler alone:
//   c++ -std=c++17 tests/cpp/test_locate_host.cpp surikatoko_amd/csrc/srk_locate.cpp
// Usage:
//   test_locate_host unit               the argument checks, the option defaults, srk_ransac_hypotheses; exit status 0 = all hold
//   test_locate_host sampler OUT S N H  the ranks of hypotheses 0 .. H - 1 among N observations under seed S: int64 [H][4]
//   test_locate_host p3p IN OUT         IN: int64 { count }, double { f0 }, K [9], X [count][3][3], uv [count][3][2].  OUT: R
//                                       [count][4][9], T [count][4][3] (doubles), ok [count][4] (int32): every root's pose
//   test_locate_host frames IN OUT      IN: int64 { n_frames, n_obs, n_points, has_q, hypotheses, seed }, double { f0, tau }, then
//                                       row_ptr (int64), point (int32), uv, q (if has_q), X, K [n][9] as raw arrays.  OUT: R [n][9],
//                                       T [n][3], located [n][6], scores [n][hypotheses] (doubles), status [n] (uint32), inliers
//                                       [n_obs] (uint8): every frame walked on the host in the kernels' order (srk_locate_host_frame)
#include "../../surikatoko_amd/csrc/srk_locate.hpp"
#include "../../surikatoko_amd/csrc/srk_locate_math.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
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
    srk_locate_options o;
    std::memset(&o, 0xff, sizeof o);
    srk_locate_default_options(&o);
    expect(o.hypotheses == 256 && o.inlier_pixels == 4.0 && o.seed == 1, "default options");
    expect(srk_locate_effective_options(nullptr).hypotheses == 256, "NULL options = the defaults");
    o.hypotheses = 7;
    expect(srk_locate_effective_options(&o).hypotheses == 7, "given options are taken");
    srk_locate_default_options(&o);
    srk_resect_options ro = { 10, 1e-9, 0, 0.0 };

    // the reference's RansacIterationsCount
    expect(srk_ransac_hypotheses(4, 0.3, 0.999) == 26 && srk_ransac_hypotheses(4, 0.5, 0.99) == 72, "the two worked values");
    expect(srk_ransac_hypotheses(4, 0.0, 0.99) == 1, "no outliers: one sample");
    expect(srk_ransac_hypotheses(4, 1.0, 0.99) == SRK_E_ARGS && srk_ransac_hypotheses(4, -0.1, 0.99) == SRK_E_ARGS &&
               srk_ransac_hypotheses(4, nan, 0.99) == SRK_E_ARGS,
           "outlier ratio outside [0, 1)");
    expect(srk_ransac_hypotheses(4, 0.3, 0.0) == SRK_E_ARGS && srk_ransac_hypotheses(4, 0.3, 1.0) == SRK_E_ARGS &&
               srk_ransac_hypotheses(4, 0.3, nan) == SRK_E_ARGS && srk_ransac_hypotheses(0, 0.3, 0.9) == SRK_E_ARGS,
           "probability outside (0, 1), empty sample");

    // a good batch: frames of 0, 1 and 3 observations over 4 landmarks
    const int64_t rp[] = { 0, 0, 1, 4 };
    const int32_t pt[] = { 3, 0, 1, 2 };
    const double uv[] = { 1, 2, 3, 4, 5, 6, 7, 8 };
    const double q[] = { 1, 0, 2.5, 1 };
    const double X[] = { 0, 0, 5, 1, 0, 5, 0, 1, 5, 1, 1, 6 };
    const double I3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    double K[27];
    for (int j = 0; j < 3; ++j) std::memcpy(K + 9 * j, I3, sizeof I3);
    auto chk = [&](int32_t n, const int64_t* a, const int32_t* b, const double* c, const double* d, int64_t np, const double* x, const double* k,
                   int shared, const srk_locate_options* op, const srk_resect_options* rf) {
        return srk_locate_check(n, a, b, c, d, np, x, k, shared, op, rf);
    };
    expect(chk(3, rp, pt, uv, q, 4, X, K, 0, &o, &ro).empty(), "a good batch passes");
    expect(chk(3, rp, pt, uv, nullptr, 4, X, K, 1, nullptr, nullptr).empty(), "q, options and refine may be NULL, K may be shared");
    expect(chk(0, rp, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr).empty(), "no frames, no arrays");
    expect(refused(chk(-1, rp, pt, uv, q, 4, X, K, 0, &o, nullptr), "negative frame count"), "negative count");
    expect(refused(chk(3, nullptr, pt, uv, q, 4, X, K, 0, &o, nullptr), "row_ptr is NULL"), "NULL row_ptr");
    expect(refused(chk(3, rp, nullptr, uv, q, 4, X, K, 0, &o, nullptr), "NULL observation array"), "NULL point");
    expect(refused(chk(3, rp, pt, nullptr, q, 4, X, K, 0, &o, nullptr), "NULL observation array"), "NULL uv");
    expect(refused(chk(3, rp, pt, uv, q, 4, X, nullptr, 0, &o, nullptr), "intrinsics array is NULL"), "NULL K");
    {
        const char* why = nullptr;
        expect(srk_locate_check_frames(3, rp, pt, uv, q, 4, nullptr, K, 0, &o, nullptr, &why) == SRK_E_ARGS && std::strstr(why, "landmark array is NULL"),
               "NULL X with a positive count");
        expect(srk_locate_check_frames(3, rp, pt, uv, q, 4, X, K, 0, &o, &ro, &why) == SRK_OK && why && !*why, "C entry: fine");
        expect(srk_locate_check_frames(3, rp, pt, uv, q, 3, X, K, 0, &o, nullptr, nullptr) == SRK_E_ARGS, "C entry: why may be NULL");
    }
    {
        const int64_t bad[] = { 1, 1, 2, 4 }, dec[] = { 0, 2, 1, 4 };
        expect(refused(chk(3, bad, pt, uv, q, 4, X, K, 0, &o, nullptr), "row_ptr[0]"), "row_ptr starts at 0");
        expect(refused(chk(3, dec, pt, uv, q, 4, X, K, 0, &o, nullptr), "decreases at frame 1"), "decreasing row_ptr");
        const int32_t hi[] = { 3, 0, 4, 2 }, lo[] = { 3, -1, 1, 2 };
        expect(refused(chk(3, rp, hi, uv, q, 4, X, K, 0, &o, nullptr), "observation 2 is out of range"), "point == n_points");
        expect(refused(chk(3, rp, lo, uv, q, 4, X, K, 0, &o, nullptr), "observation 1 is out of range"), "negative point");
    }
    for (double bad : { nan, inf }) {
        double m[8], w[4], x[12], k[27];
        std::memcpy(m, uv, sizeof m), std::memcpy(w, q, sizeof w), std::memcpy(x, X, sizeof x), std::memcpy(k, K, sizeof k);
        m[5] = bad, w[3] = bad, x[7] = bad, k[13] = bad;
        expect(refused(chk(3, rp, pt, m, q, 4, X, K, 0, &o, nullptr), "uv of observation 2"), "uv not finite");
        expect(refused(chk(3, rp, pt, uv, w, 4, X, K, 0, &o, nullptr), "q of observation 3"), "q not finite");
        expect(refused(chk(3, rp, pt, uv, q, 4, x, K, 0, &o, nullptr), "landmark 2 is not finite"), "X not finite");
        expect(refused(chk(3, rp, pt, uv, q, 4, X, k, 0, &o, nullptr), "K of frame 1 is not finite"), "K not finite");
        expect(chk(3, rp, pt, uv, q, 4, X, k, 1, &o, nullptr).empty(), "a shared K is one matrix");
        srk_locate_options b = o;
        b.inlier_pixels = bad;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, &b, nullptr), "inlier_pixels"), "tau not finite");
    }
    {
        double w[4], k[27];
        std::memcpy(w, q, sizeof w), std::memcpy(k, K, sizeof k);
        w[3] = -1e-300;
        expect(refused(chk(3, rp, pt, uv, w, 4, X, K, 0, &o, nullptr), "q of observation 3"), "negative q");
        k[18 + 8] = 0.0; // the last frame's K loses its rank
        expect(refused(chk(3, rp, pt, uv, q, 4, X, k, 0, &o, nullptr), "K of frame 2 is singular"), "singular K");
        k[18 + 8] = 1.0, k[18 + 3] = 1.0, k[18 + 1] = 1.0, k[18 + 4] = 1.0; // two equal rows
        expect(refused(chk(3, rp, pt, uv, q, 4, X, k, 0, &o, nullptr), "K of frame 2 is singular"), "rank-two K");
        srk_locate_options b = o;
        b.hypotheses = 0;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, &b, nullptr), "hypotheses outside 1..4096"), "no hypotheses");
        b.hypotheses = 4097;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, &b, nullptr), "hypotheses outside 1..4096"), "too many hypotheses");
        b.hypotheses = 4096;
        expect(chk(3, rp, pt, uv, q, 4, X, K, 0, &b, nullptr).empty(), "4096 hypotheses pass");
        b = o, b.inlier_pixels = 0.0;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, &b, nullptr), "inlier_pixels"), "tau = 0");
        b.inlier_pixels = -1.0;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, &b, nullptr), "inlier_pixels"), "tau < 0");
        srk_resect_options r = ro;
        r.attempts = 65;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, &o, &r), "refine attempts"), "refine attempts");
        r = ro, r.rel_change = -1.0;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, &o, &r), "refine rel_change"), "refine rel_change");
        r = ro, r.loss_kind = 3;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, &o, &r), "refine loss_kind"), "refine loss kind");
        r = ro, r.loss_kind = 2;
        expect(refused(chk(3, rp, pt, uv, q, 4, X, K, 0, &o, &r), "refine loss needs"), "refine loss without delta");
    }
    {   // the landmark map of the resident form
        const int64_t to_int[] = { 2, 3, 0, 1 };
        std::vector<int32_t> mapped;
        expect(srk_locate_check(3, rp, pt, uv, q, 4, nullptr, K, 0, &o, nullptr, to_int, &mapped).empty() && mapped.size() == 4 && mapped[0] == 1 &&
                   mapped[1] == 2 && mapped[2] == 3 && mapped[3] == 0,
               "points mapped through the handle's order");
    }
    {   // a frame of three weighted observations is FEW_POINTS: (I, 0) and the NaNs
        double R[9], T[3], loc[6];
        uint8_t inl[4] = { 9, 9, 9, 9 };
        const uint32_t st = srk_locate_host_frame(4, pt, uv, q, X, K, 1.0, o, R, T, loc, inl);
        expect(st == SRK_LOCATE_FEW_POINTS && R[0] == 1 && R[4] == 1 && R[8] == 1 && R[1] == 0 && T[0] == 0 && T[2] == 0, "few points: (I, 0)");
        expect(std::isnan(loc[0]) && loc[1] == 3 && loc[2] == 0 && std::isnan(loc[3]) && loc[4] == 0 && std::isnan(loc[5]), "few points: located");
        expect(inl[0] == 0 && inl[1] == 0 && inl[2] == 0 && inl[3] == 0, "few points: no inliers");
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}

template <class V> bool get(std::FILE* f, std::vector<V>& v, size_t n)
{
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(V), n, f) == n;
}
template <class V> void put(std::FILE* f, const std::vector<V>& v)
{
    if (!v.empty()) std::fwrite(v.data(), sizeof(V), v.size(), f);
}

int sampler(const char* out, uint64_t seed, int64_t n, int32_t H)
{
    std::vector<int64_t> r((size_t)(4 * H));
    for (int32_t h = 0; h < H; ++h) srk_locate_sample(seed, (uint32_t)h, n, r[4 * h], r[4 * h + 1], r[4 * h + 2], r[4 * h + 3]);
    std::FILE* f = std::fopen(out, "wb");
    if (!f) return 2;
    put(f, r);
    return std::fclose(f) ? 2 : 0;
}

int p3p(const char* in, const char* out)
{
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    std::vector<int64_t> hd;
    std::vector<double> f0, K, X, uv;
    if (!get(f, hd, 1) || !get(f, f0, 1) || !get(f, K, 9) || !get(f, X, (size_t)(9 * hd[0])) || !get(f, uv, (size_t)(6 * hd[0]))) return 2;
    std::fclose(f);
    const int64_t n = hd[0];
    std::vector<double> R((size_t)(36 * n)), T((size_t)(12 * n));
    std::vector<int32_t> ok((size_t)(4 * n));
    for (int64_t i = 0; i < n; ++i) {
        int k[4];
        srk_locate_p3p_all(K.data(), f0[0], &X[(size_t)(9 * i)], &uv[(size_t)(6 * i)], &R[(size_t)(36 * i)], &T[(size_t)(12 * i)], k);
        for (int e = 0; e < 4; ++e) ok[(size_t)(4 * i + e)] = k[e];
    }
    f = std::fopen(out, "wb");
    if (!f) return 2;
    put(f, R), put(f, T), put(f, ok);
    return std::fclose(f) ? 2 : 0;
}

int frames(const char* in, const char* out)
{
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    std::vector<int64_t> hd, rp;
    std::vector<double> sc, uv, q, X, K;
    std::vector<int32_t> pt;
    if (!get(f, hd, 6) || !get(f, sc, 2)) return 2;
    const int64_t n = hd[0], O = hd[1], N = hd[2], H = hd[4];
    if (!get(f, rp, (size_t)(n + 1)) || !get(f, pt, (size_t)O) || !get(f, uv, (size_t)(2 * O)) || (hd[3] && !get(f, q, (size_t)O)) ||
        !get(f, X, (size_t)(3 * N)) || !get(f, K, (size_t)(9 * n)))
        return 2;
    std::fclose(f);
    srk_locate_options o = { (int32_t)H, sc[1], (uint64_t)hd[5] };
    const std::string why = srk_locate_check((int32_t)n, rp.data(), pt.data(), uv.data(), hd[3] ? q.data() : nullptr, N, X.data(), K.data(), 0, &o, nullptr);
    if (!why.empty()) {
        std::fprintf(stderr, "%s\n", why.c_str());
        return 3;
    }
    std::vector<double> R((size_t)(9 * n)), T((size_t)(3 * n)), loc((size_t)(6 * n)), scores;
    std::vector<uint32_t> st((size_t)n);
    std::vector<uint8_t> inl((size_t)O);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t o0 = rp[(size_t)i];
        std::vector<double> s;
        st[(size_t)i] = srk_locate_host_frame(rp[(size_t)i + 1] - o0, pt.data() + o0, uv.data() + 2 * o0, hd[3] ? q.data() + o0 : nullptr, X.data(),
                                              &K[(size_t)(9 * i)], sc[0], o, &R[(size_t)(9 * i)], &T[(size_t)(3 * i)], &loc[(size_t)(6 * i)],
                                              inl.data() + o0, &s);
        scores.insert(scores.end(), s.begin(), s.end());
    }
    f = std::fopen(out, "wb");
    if (!f) return 2;
    put(f, R), put(f, T), put(f, loc), put(f, scores), put(f, st), put(f, inl);
    return std::fclose(f) ? 2 : 0;
}
} // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "unit") return unit();
    if (mode == "sampler" && argc == 6) return sampler(argv[2], std::strtoull(argv[3], nullptr, 10), std::atoll(argv[4]), std::atoi(argv[5]));
    if (mode == "p3p" && argc == 4) return p3p(argv[2], argv[3]);
    if (mode == "frames" && argc == 4) return frames(argv[2], argv[3]);
    std::fprintf(stderr, "usage: test_locate_host unit | sampler OUT SEED N H | p3p IN OUT | frames IN OUT\n");
    return 2;
}
