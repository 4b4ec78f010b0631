// test_pair_host.cpp -- the host half of two-view pose refinement (surikatoko_amd/csrc/srk_pair.cpp) without a GPU, driven by
// tests/test_pair_cpu.py.  Built with the host compiler alone:
//   c++ -std=c++17 tests/cpp/test_pair_host.cpp surikatoko_amd/csrc/srk_pair.cpp
// Usage:
//   test_pair_host unit    the option defaults, one refusal per rule of the checks, and walks of a synthetic pair on the host
//                          (evaluate only, q = 0 in between, every loss, the factor helper); prints "<n> failure(s)", exit status
//                          0 = all hold
#include "../../surikatoko_amd/csrc/srk_pair.hpp"
#include "../../surikatoko_amd/csrc/srk_pair_math.hpp"

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

// a small generator of its own: the walks below need matches, not statistics
struct Lcg {
    uint64_t s;
    double next() // uniform in [0, 1)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) * (1.0 / 9007199254740992.0);
    }
};

const double K0[9] = { 1.25, 0.0, 0.53, 0.0, 1.3, 0.4, 0.0, 0.0, 1.0 }, K1[9] = { 1.1, 0.01, 0.5, 0.0, 1.15, 0.42, 0.0, 0.0, 1.0 };
const double F0 = 600.0;

void pixel(const double* K, const double* x, double* uv)
{
    const double p = K[0] * x[0] + K[1] * x[1] + K[2] * x[2], q = K[3] * x[0] + K[4] * x[1] + K[5] * x[2], r = K[6] * x[0] + K[7] * x[1] + K[8] * x[2];
    uv[0] = F0 * p / r;
    uv[1] = F0 * q / r;
}

// n matches of a pose (R, T) with a little noise, and the start a few degrees off
struct Pair {
    std::vector<double> ua, ub;
    double R[9], T[3], R0[9], T0[3];
};
Pair make_pair(int n, uint64_t seed)
{
    Pair p;
    Lcg g{ seed };
    const double w[3] = { 0.05, -0.12, 0.04 }, w0[3] = { 0.03, 0.02, -0.03 };
    srk_resect_exp(w, p.R);
    double t[3] = { 0.55, 0.75, 0.36 };
    const double in = 1.0 / std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    for (int a = 0; a < 3; ++a) p.T[a] = t[a] * in;
    SrkPairPose truth, start;
    srk_pair_start_pose(p.R, p.T, 0, truth);
    const double d[5] = { w0[0], w0[1], w0[2], 0.06, -0.05 };
    srk_pair_move(truth, d, start);
    std::memcpy(p.R0, start.R, sizeof p.R0), std::memcpy(p.T0, start.T, sizeof p.T0);
    for (int k = 0; k < n; ++k) {
        const double X[3] = { 4.0 * g.next() - 2.0, 3.0 * g.next() - 1.5, 4.0 + 4.0 * g.next() };
        double Y[3], a[2], b[2];
        for (int i = 0; i < 3; ++i) Y[i] = p.R[3 * i] * X[0] + p.R[3 * i + 1] * X[1] + p.R[3 * i + 2] * X[2] + p.T[i];
        pixel(K0, X, a), pixel(K1, Y, b);
        p.ua.push_back(a[0] + g.next() - 0.5), p.ua.push_back(a[1] + g.next() - 0.5);
        p.ub.push_back(b[0] + g.next() - 0.5), p.ub.push_back(b[1] + g.next() - 0.5);
    }
    return p;
}

struct Out {
    double R[9], T[3], E[9], quality[6], info[25], basis[6], grad[5];
    std::vector<double> w;
    std::vector<SrkPairAttempt> log;
    uint32_t status;
};
Out walk(const Pair& p, const double* q, const srk_pair_options& o, const std::vector<double>* ua = nullptr, const std::vector<double>* ub = nullptr)
{
    const std::vector<double>& a = ua ? *ua : p.ua;
    const std::vector<double>& b = ub ? *ub : p.ub;
    Out r;
    r.w.assign(a.size() / 2, -1.0);
    r.status = srk_pair_host_pair_cpp((int64_t)(a.size() / 2), a.data(), b.data(), q, K0, K1, F0, p.R0, p.T0, o, r.R, r.T, r.E, r.quality, r.info, r.basis,
                                      r.w.data(), r.grad, &r.log);
    return r;
}
bool same(const void* a, const void* b, size_t bytes) { return std::memcmp(a, b, bytes) == 0; }
bool same_pose(const Out& a, const Out& b)
{
    return same(a.R, b.R, sizeof a.R) && same(a.T, b.T, sizeof a.T) && same(a.E, b.E, sizeof a.E) && same(a.quality, b.quality, sizeof a.quality) &&
           same(a.info, b.info, sizeof a.info) && same(a.basis, b.basis, sizeof a.basis) && a.status == b.status;
}

void unit_checks()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    srk_pair_options o;
    std::memset(&o, 0xff, sizeof o);
    srk_pair_default_options(&o);
    expect(o.attempts == 10 && o.rel_change == 1e-9 && o.loss_kind == 0 && o.loss_delta_pixels == 0.0 && o.inliers_only == 0, "default options");
    expect(srk_pair_effective_options(nullptr).attempts == 10, "NULL options = the defaults");
    o.attempts = 7;
    expect(srk_pair_effective_options(&o).attempts == 7, "given options are taken");
    srk_pair_default_options(&o);

    // a good batch: pairs of 0, 1 and 3 matches
    const int64_t rp[] = { 0, 0, 1, 4 };
    const double ua[] = { 1, 2, 3, 4, 5, 6, 7, 8 }, ub[] = { 2, 1, 4, 3, 6, 5, 8, 7 };
    const double q[] = { 1, 0, 2.5, 1 };
    const double I3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    double K[27], R[27], T[9] = { 1, 0, 0, 0, 1, 0, 0, 0.6, 0.8 };
    for (int j = 0; j < 3; ++j) std::memcpy(K + 9 * j, I3, sizeof I3), std::memcpy(R + 9 * j, I3, sizeof I3);
    auto chk = srk_pair_check;
    expect(chk(3, rp, ua, ub, q, K, K, 0, R, T, &o).empty(), "a good batch passes");
    expect(chk(3, rp, ua, ub, nullptr, K, K, 1, R, T, nullptr).empty(), "q and options may be NULL, K may be shared");
    expect(chk(0, rp, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr).empty(), "no pairs, no arrays");
    expect(refused(chk(-1, rp, ua, ub, q, K, K, 0, R, T, &o), "negative pair count"), "negative count");
    expect(refused(chk(3, nullptr, ua, ub, q, K, K, 0, R, T, &o), "row_ptr is NULL"), "NULL row_ptr");
    expect(refused(chk(3, rp, nullptr, ub, q, K, K, 0, R, T, &o), "NULL match array"), "NULL uv_a");
    expect(refused(chk(3, rp, ua, nullptr, q, K, K, 0, R, T, &o), "NULL match array"), "NULL uv_b");
    expect(refused(chk(3, rp, ua, ub, q, nullptr, K, 0, R, T, &o), "intrinsics array is NULL"), "NULL K_a");
    expect(refused(chk(3, rp, ua, ub, q, K, nullptr, 0, R, T, &o), "intrinsics array is NULL"), "NULL K_b");
    expect(refused(chk(3, rp, ua, ub, q, K, K, 0, nullptr, T, &o), "NULL start pose"), "NULL R0");
    expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, nullptr, &o), "NULL start pose"), "NULL T0");
    {
        const char* why = nullptr;
        expect(srk_pair_check_pairs(3, rp, ua, ub, q, K, K, 0, R, T, &o, &why) == SRK_OK && why && !*why, "C entry: fine");
        expect(srk_pair_check_pairs(3, rp, ua, ub, q, K, nullptr, 0, R, T, &o, &why) == SRK_E_ARGS && std::strstr(why, "intrinsics"), "C entry: refused");
        expect(srk_pair_check_pairs(3, rp, ua, ub, q, K, nullptr, 0, R, T, &o, nullptr) == SRK_E_ARGS, "C entry: why may be NULL");
    }
    {
        const int64_t bad[] = { 1, 1, 2, 4 }, dec[] = { 0, 2, 1, 4 }, neg[] = { 0, -1, 1, 4 };
        expect(refused(chk(3, bad, ua, ub, q, K, K, 0, R, T, &o), "row_ptr[0]"), "row_ptr starts at 0");
        expect(refused(chk(3, dec, ua, ub, q, K, K, 0, R, T, &o), "decreases at pair 1"), "decreasing row_ptr");
        expect(refused(chk(3, neg, ua, ub, q, K, K, 0, R, T, &o), "decreases at pair 0"), "negative row_ptr");
    }
    for (double bad : { nan, inf }) {
        double m[8], w[4], k[27], r[27], t[9];
        std::memcpy(m, ua, sizeof m), std::memcpy(w, q, sizeof w), std::memcpy(k, K, sizeof k), std::memcpy(r, R, sizeof r), std::memcpy(t, T, sizeof t);
        m[5] = bad, w[3] = bad, k[13] = bad, r[20] = bad, t[4] = bad;
        expect(refused(chk(3, rp, m, ub, q, K, K, 0, R, T, &o), "uv_a of match 2"), "uv_a not finite");
        expect(refused(chk(3, rp, ua, m, q, K, K, 0, R, T, &o), "uv_b of match 2"), "uv_b not finite");
        expect(refused(chk(3, rp, ua, ub, w, K, K, 0, R, T, &o), "q of match 3"), "q not finite");
        expect(refused(chk(3, rp, ua, ub, q, k, K, 0, R, T, &o), "K_a of pair 1 is not finite"), "K_a not finite");
        expect(refused(chk(3, rp, ua, ub, q, K, k, 0, R, T, &o), "K_b of pair 1 is not finite"), "K_b not finite");
        expect(chk(3, rp, ua, ub, q, K, k, 1, R, T, &o).empty(), "a shared K is one matrix");
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, r, T, &o), "R0 of pair 2 is not finite"), "R0 not finite");
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, t, &o), "T0 of pair 1 is not finite"), "T0 not finite");
        srk_pair_options b = o;
        b.rel_change = bad;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, T, &b), "rel_change"), "rel_change not finite");
        b = o, b.loss_kind = 1, b.loss_delta_pixels = bad;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, T, &b), "loss_delta_pixels"), "delta not finite");
    }
    {
        double w[4], k[27], r[27], t[9];
        std::memcpy(w, q, sizeof w), std::memcpy(k, K, sizeof k), std::memcpy(r, R, sizeof r), std::memcpy(t, T, sizeof t);
        w[2] = -1.0;
        expect(refused(chk(3, rp, ua, ub, w, K, K, 0, R, T, &o), "q of match 2"), "negative q");
        k[9 + 8] = 0.0;
        expect(refused(chk(3, rp, ua, ub, q, K, k, 0, R, T, &o), "K_b of pair 1 is singular"), "singular K");
        r[9] = 1.0 + 1e-8;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, r, T, &o), "R0 of pair 1 is not orthogonal"), "R0 not orthogonal");
        std::memcpy(r, R, sizeof r);
        r[18] = -1.0; // a reflection
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, r, T, &o), "R0 of pair 2 has determinant"), "R0 a reflection");
        t[6] = 1e-8;
        expect(chk(3, rp, ua, ub, q, K, K, 0, R, t, &o).empty(), "T0 of length 1 to 1e-9 passes");
        t[7] = 0.61;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, t, &o), "T0 of pair 2 is not a unit vector"), "T0 not unit");
        t[7] = t[8] = 0.0, t[6] = 0.0;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, t, &o), "T0 of pair 2 is not a unit vector"), "T0 zero");
    }
    {
        srk_pair_options b = o;
        b.attempts = -1;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, T, &b), "attempts outside 0..64"), "attempts < 0");
        b.attempts = 65;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, T, &b), "attempts outside 0..64"), "attempts > 64");
        b.attempts = 64;
        expect(chk(3, rp, ua, ub, q, K, K, 0, R, T, &b).empty(), "64 attempts pass");
        b = o, b.rel_change = -1e-9;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, T, &b), "rel_change"), "negative rel_change");
        b = o, b.loss_kind = 3;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, T, &b), "loss_kind outside 0..2"), "loss kind 3");
        b.loss_kind = -1;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, T, &b), "loss_kind outside 0..2"), "loss kind -1");
        b = o, b.loss_kind = 2, b.loss_delta_pixels = 0.0;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, T, &b), "loss_delta_pixels"), "a loss without delta");
        b = o, b.inliers_only = 2;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, T, &b), "inliers_only must be 0 or 1"), "inliers_only 2");
        expect(refused(srk_pair_check_options(&b, true), "inliers_only must be 0 or 1"), "inliers_only 2, chained");
        b.inliers_only = 1;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, R, T, &b), "inliers_only has no meaning"), "inliers_only 1 without relate");
        expect(srk_pair_check_options(&b, true).empty(), "inliers_only 1 in the chained call");
    }
}

void unit_walks()
{
    const Pair p = make_pair(150, 7);
    srk_pair_options o;
    srk_pair_default_options(&o);
    // evaluate only: the start comes back bit for bit
    o.attempts = 0;
    const Out start = walk(p, nullptr, o);
    expect(same(start.R, p.R0, sizeof p.R0) && same(start.T, p.T0, sizeof p.T0) && start.quality[5] == 0.0 && start.log.empty(), "attempts 0 returns the start");
    expect(!(start.status & SRK_PAIR_NOT_CONVERGED), "evaluate only is not 'not converged'");
    // the defaults converge, E_pair never grows, the pose nears the truth
    srk_pair_default_options(&o);
    for (int kind = 0; kind < 3; ++kind) {
        o.loss_kind = kind, o.loss_delta_pixels = kind ? 1.0 : 0.0;
        srk_pair_options e = o;
        e.attempts = 0;
        const Out s0 = walk(p, nullptr, e), r = walk(p, nullptr, o);
        expect(r.quality[0] <= s0.quality[0], "E_out <= E_start");
        expect(r.quality[0] < 1.0 && r.quality[1] == 150.0 && r.quality[4] == 150.0, "the refined pair fits its matches, all in front");
        double dr = 0.0, dt = 0.0;
        for (int k = 0; k < 9; ++k) dr = std::fmax(dr, std::fabs(r.R[k] - p.R[k]));
        for (int k = 0; k < 3; ++k) dt = std::fmax(dt, std::fabs(r.T[k] - p.T[k]));
        expect(dr < 5e-3 && dt < 2e-2, "the pose nears the truth");
        expect(std::fabs(r.T[0] * r.T[0] + r.T[1] * r.T[1] + r.T[2] * r.T[2] - 1.0) < 1e-15, "T is a unit vector");
        double E[9];
        srk_relate_essential(r.R, r.T, E);
        expect(same(E, r.E, sizeof E), "E = [T]x R exactly as returned");
        for (const SrkPairAttempt& a : r.log) expect(a.accepted ? a.E_cand < a.E_cur : !(a.E_cand < a.E_cur), "accepted iff E_pair decreases");
        for (double w : r.w) expect(w > 0.0 && w <= 1.0, "robust weights in (0, 1]");
    }
    // q = 0 is the pair without the match, bit for bit; q all 1 is q NULL
    {
        std::vector<double> q(150, 1.0), ua, ub, qs;
        Lcg g{ 11 };
        for (int k = 0; k < 150; ++k) {
            q[(size_t)k] = g.next() < 0.2 ? 0.0 : 0.5 + 1.5 * g.next();
            if (q[(size_t)k] > 0.0) {
                ua.push_back(p.ua[2 * (size_t)k]), ua.push_back(p.ua[2 * (size_t)k + 1]);
                ub.push_back(p.ub[2 * (size_t)k]), ub.push_back(p.ub[2 * (size_t)k + 1]);
                qs.push_back(q[(size_t)k]);
            }
        }
        o.loss_kind = 2, o.loss_delta_pixels = 1.0, o.attempts = 4;
        const Out a = walk(p, q.data(), o), b = walk(p, qs.data(), o, &ua, &ub);
        expect(same_pose(a, b), "q = 0 leaves the bits of the pair without the match");
        size_t j = 0;
        bool w_ok = true;
        for (int k = 0; k < 150; ++k) w_ok = w_ok && (q[(size_t)k] > 0.0 ? same(&a.w[(size_t)k], &b.w[j++], 8) : a.w[(size_t)k] == 0.0);
        expect(w_ok, "w_out is 0 where q = 0 and the short pair's elsewhere");
        const std::vector<double> ones(150, 1.0);
        expect(same_pose(walk(p, ones.data(), o), walk(p, nullptr, o)), "q all 1 is q NULL");
    }
    // status words
    {
        srk_pair_default_options(&o);
        const Pair few = make_pair(4, 3);
        const Out f = walk(few, nullptr, o);
        expect(f.status == SRK_PAIR_FEW_POINTS && std::isnan(f.quality[3]) && same(f.R, few.R0, sizeof f.R) && same(f.T, few.T0, sizeof f.T), "four matches: FEW_POINTS");
        o.attempts = 1;
        expect(walk(p, nullptr, o).status == SRK_PAIR_NOT_CONVERGED, "one attempt from the off start: NOT_CONVERGED");
        Pair c = make_pair(1, 5);
        for (int k = 1; k < 8; ++k) c.ua.push_back(c.ua[0]), c.ua.push_back(c.ua[1]), c.ub.push_back(c.ub[0]), c.ub.push_back(c.ub[1]);
        o.attempts = 2;
        const Out d = walk(c, nullptr, o);
        expect((d.status & SRK_PAIR_DEGENERATE) || d.quality[3] >= 1e12, "eight copies of one match: DEGENERATE or cond_1 >= 1e12");
    }
    // the factor helper: the null direction and the refusals
    {
        srk_pair_default_options(&o);
        const Out r = walk(p, nullptr, o);
        double Z[9], z[3], L21[21], L[6][6];
        expect(srk_pair_factor(r.R, r.T, r.info, r.basis, 2.5, Z, z, L21) == SRK_OK, "factor: fine");
        int e = 0;
        double big = 0.0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) L[a][b] = L[b][a] = L21[e++], big = std::fmax(big, std::fabs(L[a][b]));
        for (int a = 0; a < 6; ++a) expect(std::fabs(L[a][0] * z[0] + L[a][1] * z[1] + L[a][2] * z[2]) <= 1e-12 * big * 2.5, "factor: L [z; 0] = 0");
        expect(std::fabs(std::sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]) - 2.5) < 1e-14 && Z[1] == r.R[3], "factor: z has the baseline's length, Z = R^T");
        expect(srk_pair_factor(r.R, r.T, r.info, r.basis, 0.0, Z, z, L21) == SRK_E_ARGS, "factor: baseline 0");
        expect(srk_pair_factor(r.R, r.T, r.info, r.basis, std::numeric_limits<double>::infinity(), Z, z, L21) == SRK_E_ARGS, "factor: baseline inf");
        expect(srk_pair_factor(nullptr, r.T, r.info, r.basis, 1.0, Z, z, L21) == SRK_E_ARGS, "factor: NULL R");
        expect(srk_pair_factor(r.R, r.T, r.info, r.basis, 1.0, Z, z, nullptr) == SRK_E_ARGS, "factor: NULL output");
    }
    // the C entry of the walk
    {
        srk_pair_default_options(&o);
        const Out r = walk(p, nullptr, o);
        double R[9], T[3], E[9], ql[6], inf[25], bs[6], gr[5], log[30];
        int32_t count = -1;
        const int st = srk_pair_host_pair(150, p.ua.data(), p.ub.data(), nullptr, K0, K1, F0, p.R0, p.T0, &o, R, T, E, ql, inf, bs, nullptr, gr, log, &count);
        expect(st == (int)r.status && same(R, r.R, sizeof R) && same(T, r.T, sizeof T) && count == (int32_t)r.log.size() && same(gr, r.grad, sizeof gr), "C entry of the walk");
        expect(srk_pair_host_pair(150, p.ua.data(), p.ub.data(), nullptr, K0, K1, 0.0, p.R0, p.T0, &o, R, T, E, ql, inf, bs, nullptr, nullptr, nullptr, nullptr) == SRK_E_ARGS,
               "C entry: f0 = 0");
    }
}
} // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && std::strcmp(argv[1], "unit") == 0) {
        unit_checks();
        unit_walks();
        std::printf("%d failure(s)\n", failures);
        return failures ? 1 : 0;
    }
    std::fprintf(stderr, "usage: test_pair_host unit\n");
    return 2;
}
