// test_align_host.cpp -- the host half of map alignment (surikatoko_amd/csrc/srk_align.cpp) without a GPU, driven by
// tests/test_align_cpu.py.  Built with the host compiler alone:
//   c++ -std=c++17 tests/cpp/test_align_host.cpp surikatoko_amd/csrc/srk_align.cpp
// Usage:
//   test_align_host unit               the argument checks, the option defaults, a walk of three sets and srk_similarity_apply;
//                                      exit status 0 = all hold
//   test_align_host sampler OUT S N H  the ranks of hypotheses 0 .. H - 1 among N correspondences under seed S: int64 [H][3]
#include "../../surikatoko_amd/csrc/srk_align.hpp"
#include "../../surikatoko_amd/csrc/srk_align_math.hpp"

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

// a fixed linear congruential stream in [-1, 1): the unit test needs no more
struct Lcg {
    uint64_t x = 12345;
    double next()
    {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(x >> 11) / 4503599627370496.0 - 1.0;
    }
};

void map_point(double s, const double* R, const double* t, const double* a, double* b)
{
    for (int r = 0; r < 3; ++r) b[r] = s * (R[3 * r] * a[0] + R[3 * r + 1] * a[1] + R[3 * r + 2] * a[2]) + t[r];
}

int unit()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    srk_align_options o;
    std::memset(&o, 0xff, sizeof o);
    srk_align_default_options(&o);
    expect(o.hypotheses == 256 && o.inlier_distance == 0.0 && o.seed == 1 && o.with_scale == 1 && o.refine_rounds == 2, "default options");
    expect(srk_align_effective_options(nullptr).hypotheses == 256, "NULL options = the defaults");

    const int64_t rp[] = { 0, 0, 1, 4 };
    const double a[] = { 1, 2, 3, 4, 5, 6, 7, 8, 9, 1, 0, 1 }, b[] = { 2, 1, 4, 3, 6, 5, 8, 7, 1, 0, 1, 0 };
    const double q[] = { 1, 0, 2.5, 1 };
    const int32_t pt[] = { 0, 5, 2, 1 };
    auto chk = [](int32_t n_sets, const int64_t* row_ptr, const int32_t* point, int64_t n_points, const double* x, const double* y, const double* w,
                  const srk_align_options* opts) { return srk_align_check(n_sets, row_ptr, point, n_points, x, y, w, opts); };
    expect(refused(chk(3, rp, nullptr, 0, a, b, q, &o), "inlier_distance"), "the default inlier_distance is refused");
    expect(refused(chk(3, rp, nullptr, 0, a, b, q, nullptr), "inlier_distance"), "and so are NULL options");
    o.inlier_distance = 0.1;
    expect(chk(3, rp, nullptr, 0, a, b, q, &o).empty(), "a good batch passes");
    expect(chk(3, rp, nullptr, 0, a, b, nullptr, &o).empty(), "q may be NULL");
    expect(chk(0, rp, nullptr, 0, nullptr, nullptr, nullptr, &o).empty(), "no sets, no arrays");
    expect(chk(3, rp, pt, 6, nullptr, b, q, &o).empty(), "landmarks of a map: a may be NULL");
    expect(refused(chk(3, rp, pt, 5, nullptr, b, q, &o), "correspondence 1 is beyond the map"), "an index beyond the map");
    expect(refused(chk(-1, rp, nullptr, 0, a, b, q, &o), "negative set count"), "negative count");
    expect(refused(chk(3, nullptr, nullptr, 0, a, b, q, &o), "row_ptr is NULL"), "NULL row_ptr");
    expect(refused(chk(3, rp, nullptr, 0, nullptr, b, q, &o), "NULL correspondence array"), "NULL a");
    expect(refused(chk(3, rp, nullptr, 0, a, nullptr, q, &o), "NULL correspondence array"), "NULL b");
    {
        const int64_t bad[] = { 1, 1, 2, 4 }, dec[] = { 0, 2, 1, 4 }, neg[] = { 0, -1, 1, 4 };
        expect(refused(chk(3, bad, nullptr, 0, a, b, q, &o), "row_ptr[0]"), "row_ptr starts at 0");
        expect(refused(chk(3, dec, nullptr, 0, a, b, q, &o), "decreases at set 1"), "decreasing row_ptr");
        expect(refused(chk(3, neg, nullptr, 0, a, b, q, &o), "decreases at set 0"), "negative row_ptr");
    }
    for (double bad : { nan, inf }) {
        double x[12], w[4];
        std::memcpy(x, a, sizeof x), std::memcpy(w, q, sizeof w);
        x[7] = bad, w[3] = bad;
        expect(refused(chk(3, rp, nullptr, 0, x, b, q, &o), "a of correspondence 2"), "a not finite");
        expect(refused(chk(3, rp, nullptr, 0, a, x, q, &o), "b of correspondence 2"), "b not finite");
        expect(refused(chk(3, rp, nullptr, 0, a, b, w, &o), "q of correspondence 3"), "q not finite");
    }
    {
        double w[4];
        std::memcpy(w, q, sizeof w);
        w[0] = -1.0;
        expect(refused(chk(3, rp, nullptr, 0, a, b, w, &o), "q of correspondence 0"), "negative q");
        srk_align_options p = o;
        p.hypotheses = 0;
        expect(refused(chk(3, rp, nullptr, 0, a, b, q, &p), "hypotheses outside 1..4096"), "no hypotheses");
        p.hypotheses = 4097;
        expect(refused(chk(3, rp, nullptr, 0, a, b, q, &p), "hypotheses outside"), "too many hypotheses");
        p = o, p.inlier_distance = inf;
        expect(refused(chk(3, rp, nullptr, 0, a, b, q, &p), "inlier_distance"), "infinite inlier_distance");
        p = o, p.refine_rounds = 17;
        expect(refused(chk(3, rp, nullptr, 0, a, b, q, &p), "refine_rounds outside 0..16"), "too many rounds");
        p = o, p.refine_rounds = -1;
        expect(refused(chk(3, rp, nullptr, 0, a, b, q, &p), "refine_rounds"), "negative rounds");
        p = o, p.with_scale = 2;
        expect(refused(chk(3, rp, nullptr, 0, a, b, q, &p), "with_scale"), "with_scale is a flag");
        p = o, p.hypotheses = 4096;
        const std::vector<int64_t> many((size_t)(1 << 16) + 2, 0);
        expect(refused(chk((1 << 16) + 1, many.data(), nullptr, 0, nullptr, nullptr, nullptr, &p), "split the batch"), "more than 2^22 waves");
        expect(chk(1 << 16, many.data(), nullptr, 0, nullptr, nullptr, nullptr, &p).empty(), "2^22 waves pass");
    }
    {
        double s[3], R[27], t[9], al[24];
        uint32_t st[3];
        const char* why = nullptr;
        expect(srk_align_check_sets(3, rp, nullptr, 0, a, b, q, &o, s, R, t, al, st, &why) == SRK_OK && why && !*why, "C entry: fine");
        expect(srk_align_check_sets(3, rp, nullptr, 0, a, b, q, &o, s, nullptr, t, al, st, &why) == SRK_E_ARGS && std::strstr(why, "NULL output"), "C entry: NULL output");
        expect(srk_align_check_sets(3, rp, nullptr, 0, a, nullptr, q, &o, s, R, t, al, st, nullptr) == SRK_E_ARGS, "C entry: why may be NULL");
    }

    // a walk: 40 points under a known similarity, eight targets wrong and four switched off; then a collinear set and a short one
    Lcg g;
    const int n = 40;
    std::vector<double> A(3 * n), B(3 * n), Q(n, 1.0);
    const double c = std::cos(0.7), sn = std::sin(0.7), Rt[9] = { c, -sn, 0, sn, c, 0, 0, 0, 1 }, tt[3] = { 0.5, -2.0, 3.0 }, st = 1.7;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) A[3 * i + k] = 2.0 * g.next();
        map_point(st, Rt, tt, &A[3 * i], &B[3 * i]);
        if (i % 5 == 0) B[3 * i + 1] += 4.0;
        if (i % 10 == 3) Q[i] = 0.0, B[3 * i] = 100.0;
    }
    srk_align_options w = o;
    w.hypotheses = 64, w.inlier_distance = 0.01;
    double s = 0, R[9], t[3], al[8];
    std::vector<uint8_t> inl(n, 7);
    std::vector<double> scores;
    uint32_t status = srk_align_host_walk(n, A.data(), B.data(), Q.data(), w, &s, R, t, al, inl.data(), &scores);
    double dr = 0;
    for (int e = 0; e < 9; ++e) dr = std::fmax(dr, std::fabs(R[e] - Rt[e]));
    expect(status == 0 && std::fabs(s / st - 1) < 1e-12 && dr < 1e-12 && std::fabs(t[0] - tt[0]) + std::fabs(t[1] - tt[1]) + std::fabs(t[2] - tt[2]) < 1e-11,
           "the walk recovers the similarity");
    expect(al[1] == 36 && al[2] == 28 && al[3] >= 0 && al[4] > 0 && scores.size() == 64, "n, the inlier count and the scores");
    for (int i = 0; i < n; ++i) expect(inl[i] == (i % 5 != 0 && i % 10 != 3), "the inlier flags");
    expect(srk_align_host_set(n, A.data(), B.data(), Q.data(), &w, &s, R, t, al, nullptr) == 0, "C entry: the walk, inlier_out may be NULL");
    w.inlier_distance = 0;
    expect(srk_align_host_set(n, A.data(), B.data(), Q.data(), &w, &s, R, t, al, nullptr) == SRK_E_ARGS, "C entry: the checks come first");
    w.inlier_distance = 0.01;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) A[3 * i + k] = (k + 1) * 0.1 * i, B[3 * i + k] = (3 - k) * 0.2 * i;
    status = srk_align_host_walk(n, A.data(), B.data(), nullptr, w, &s, R, t, al, inl.data());
    expect(status == SRK_ALIGN_NO_MODEL && s == 1.0 && R[0] == 1.0 && R[1] == 0.0 && t[2] == 0.0 && al[4] == 0 && std::isnan(al[0]), "a line has no model");
    status = srk_align_host_walk(2, A.data(), B.data(), nullptr, w, &s, R, t, al, inl.data());
    expect(status == SRK_ALIGN_FEW_POINTS && al[1] == 2 && std::isnan(al[3]) && inl[0] == 0, "two points are too few");

    // srk_similarity_apply: a point and a pose keep their camera coordinates up to the scale, and the inverse undoes it
    double X[3] = { 0.3, -1.0, 2.0 }, cR[9] = { 0, -1, 0, 1, 0, 0, 0, 0, 1 }, cT[3] = { 0.1, 0.2, 4.0 }, before[3], after[3];
    for (int r = 0; r < 3; ++r) before[r] = cR[3 * r] * X[0] + cR[3 * r + 1] * X[1] + cR[3 * r + 2] * X[2] + cT[r];
    expect(srk_similarity_apply(st, Rt, tt, 1, X, 1, cR, cT) == SRK_OK, "apply");
    for (int r = 0; r < 3; ++r) after[r] = cR[3 * r] * X[0] + cR[3 * r + 1] * X[1] + cR[3 * r + 2] * X[2] + cT[r];
    expect(std::fabs(after[0] - st * before[0]) + std::fabs(after[1] - st * before[1]) + std::fabs(after[2] - st * before[2]) < 1e-13, "camera coordinates scale by s");
    double Ri[9], ti[3];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) Ri[3 * r + k] = Rt[3 * k + r];
    for (int r = 0; r < 3; ++r) ti[r] = -(Ri[3 * r] * tt[0] + Ri[3 * r + 1] * tt[1] + Ri[3 * r + 2] * tt[2]) / st;
    expect(srk_similarity_apply(1.0 / st, Ri, ti, 1, X, 1, cR, cT) == SRK_OK, "apply the inverse");
    expect(std::fabs(X[0] - 0.3) + std::fabs(X[1] + 1.0) + std::fabs(X[2] - 2.0) < 1e-14 && std::fabs(cT[2] - 4.0) < 1e-14 && std::fabs(cR[1] + 1.0) < 1e-15, "the round trip");
    expect(srk_similarity_apply(st, Rt, tt, 0, nullptr, 0, nullptr, nullptr) == SRK_OK, "either group may be NULL");
    expect(srk_similarity_apply(0.0, Rt, tt, 1, X, 0, nullptr, nullptr) == SRK_E_ARGS, "s must be positive");
    expect(srk_similarity_apply(st, Rt, tt, 0, nullptr, 1, cR, nullptr) == SRK_E_ARGS, "cam_R and cam_T go together");

    // the revert of the normalised scene's similarity: (sigma s_n, Q R0, sigma s_n Q T0 + tau)
    srk_ba_normalizer nrm{};
    std::memcpy(nrm.R0, Rt, sizeof Rt);
    nrm.T0[0] = 1, nrm.T0[1] = 2, nrm.T0[2] = 3, nrm.world_scale = 0.5;
    double Xc[3] = { 0.3, -1.0, 2.0 }, Xn[3], want[3], got[3];
    for (int r = 0; r < 3; ++r) Xn[r] = 0.5 * (Rt[3 * r] * Xc[0] + Rt[3 * r + 1] * Xc[1] + Rt[3 * r + 2] * Xc[2] + nrm.T0[r]);
    double sg = 3.0, Qm[9] = { 0, 0, 1, 1, 0, 0, 0, 1, 0 }, tau[3] = { -1, 0, 2 };
    map_point(sg, Qm, tau, Xn, want);
    srk_align_revert(nrm, 1, &sg, Qm, tau);
    map_point(sg, Qm, tau, Xc, got);
    expect(std::fabs(got[0] - want[0]) + std::fabs(got[1] - want[1]) + std::fabs(got[2] - want[2]) < 1e-14 && sg == 1.5, "the revert maps the caller's coordinates");

    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}

int sampler(const char* out, uint64_t seed, int64_t n, int64_t H)
{
    std::vector<int64_t> r((size_t)(3 * H));
    for (int64_t h = 0; h < H; ++h) srk_align_sample(seed, (uint32_t)h, n, r[(size_t)(3 * h)], r[(size_t)(3 * h + 1)], r[(size_t)(3 * h + 2)]);
    FILE* f = std::fopen(out, "wb");
    if (!f) return 2;
    const bool ok = std::fwrite(r.data(), 8, r.size(), f) == r.size();
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "unit")) return unit();
    if (argc == 6 && !std::strcmp(argv[1], "sampler"))
        return sampler(argv[2], std::strtoull(argv[3], nullptr, 10), std::strtoll(argv[4], nullptr, 10), std::strtoll(argv[5], nullptr, 10));
    std::fprintf(stderr, "usage: test_align_host unit | sampler OUT SEED N H\n");
    return 2;
}
