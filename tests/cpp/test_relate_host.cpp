// test_relate_host.cpp -- the host half of two-view relative pose (surikatoko_amd/csrc/srk_relate.cpp) without a GPU, driven by
// tests/test_relate_cpu.py.  Built with the host compiler alone:
//   c++ -std=c++17 tests/cpp/test_relate_host.cpp surikatoko_amd/csrc/srk_relate.cpp
// Usage:
//   test_relate_host unit               the argument checks and the option defaults; exit status 0 = all hold
//   test_relate_host sampler OUT S N H  the ranks of hypotheses 0 .. H - 1 among N matches under seed S: int64 [H][6]
//   test_relate_host solve IN OUT       IN: int64 { count }, double { f0 }, K_a [9], K_b [9], uv_a [count][6][2], uv_b [count][6][2].
//                                       OUT: E [count][10][9], rec [count][20] (doubles), roots [count] (int32): the five-point solve
//   test_relate_host poses IN OUT       IN: int64 { count }, E [count][9].  OUT: R [count][4][9], T [count][4][3]
//   test_relate_host pairs IN OUT       IN: int64 { n_pairs, n_obs, has_q, hypotheses, seed }, double { f0, tau }, then row_ptr (int64),
//                                       uv_a, uv_b, q (if has_q), K_a [n][9], K_b [n][9] as raw arrays.  OUT: R [n][9], T [n][3], E [n][9],
//                                       related [n][8], scores [n][hypotheses] (doubles), status [n] (uint32), inliers [n_obs] (uint8):
//                                       every pair walked on the host in the kernels' order
#include "../../surikatoko_amd/csrc/srk_relate.hpp"
#include "../../surikatoko_amd/csrc/srk_relate_math.hpp"

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
    srk_relate_options o;
    std::memset(&o, 0xff, sizeof o);
    srk_relate_default_options(&o);
    expect(o.hypotheses == 256 && o.inlier_pixels == 2.0 && o.seed == 1, "default options");
    expect(srk_relate_effective_options(nullptr).hypotheses == 256, "NULL options = the defaults");
    o.hypotheses = 7;
    expect(srk_relate_effective_options(&o).hypotheses == 7, "given options are taken");
    srk_relate_default_options(&o);

    // a good batch: pairs of 0, 1 and 3 matches
    const int64_t rp[] = { 0, 0, 1, 4 };
    const double ua[] = { 1, 2, 3, 4, 5, 6, 7, 8 }, ub[] = { 2, 1, 4, 3, 6, 5, 8, 7 };
    const double q[] = { 1, 0, 2.5, 1 };
    const double I3[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    double K[27];
    for (int j = 0; j < 3; ++j) std::memcpy(K + 9 * j, I3, sizeof I3);
    auto chk = srk_relate_check;
    expect(chk(3, rp, ua, ub, q, K, K, 0, &o).empty(), "a good batch passes");
    expect(chk(3, rp, ua, ub, nullptr, K, K, 1, nullptr).empty(), "q and options may be NULL, K may be shared");
    expect(chk(0, rp, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr).empty(), "no pairs, no arrays");
    expect(refused(chk(-1, rp, ua, ub, q, K, K, 0, &o), "negative pair count"), "negative count");
    expect(refused(chk(3, nullptr, ua, ub, q, K, K, 0, &o), "row_ptr is NULL"), "NULL row_ptr");
    expect(refused(chk(3, rp, nullptr, ub, q, K, K, 0, &o), "NULL match array"), "NULL uv_a");
    expect(refused(chk(3, rp, ua, nullptr, q, K, K, 0, &o), "NULL match array"), "NULL uv_b");
    expect(refused(chk(3, rp, ua, ub, q, nullptr, K, 0, &o), "intrinsics array is NULL"), "NULL K_a");
    expect(refused(chk(3, rp, ua, ub, q, K, nullptr, 0, &o), "intrinsics array is NULL"), "NULL K_b");
    {
        const char* why = nullptr;
        expect(srk_relate_check_pairs(3, rp, ua, ub, q, K, K, 0, &o, &why) == SRK_OK && why && !*why, "C entry: fine");
        expect(srk_relate_check_pairs(3, rp, ua, ub, q, K, nullptr, 0, &o, &why) == SRK_E_ARGS && std::strstr(why, "intrinsics"), "C entry: refused");
        expect(srk_relate_check_pairs(3, rp, ua, ub, q, K, nullptr, 0, &o, nullptr) == SRK_E_ARGS, "C entry: why may be NULL");
    }
    {
        const int64_t bad[] = { 1, 1, 2, 4 }, dec[] = { 0, 2, 1, 4 }, neg[] = { 0, -1, 1, 4 };
        expect(refused(chk(3, bad, ua, ub, q, K, K, 0, &o), "row_ptr[0]"), "row_ptr starts at 0");
        expect(refused(chk(3, dec, ua, ub, q, K, K, 0, &o), "decreases at pair 1"), "decreasing row_ptr");
        expect(refused(chk(3, neg, ua, ub, q, K, K, 0, &o), "decreases at pair 0"), "negative row_ptr");
    }
    for (double bad : { nan, inf }) {
        double m[8], w[4], k[27];
        std::memcpy(m, ua, sizeof m), std::memcpy(w, q, sizeof w), std::memcpy(k, K, sizeof k);
        m[5] = bad, w[3] = bad, k[13] = bad;
        expect(refused(chk(3, rp, m, ub, q, K, K, 0, &o), "uv_a of match 2"), "uv_a not finite");
        expect(refused(chk(3, rp, ua, m, q, K, K, 0, &o), "uv_b of match 2"), "uv_b not finite");
        expect(refused(chk(3, rp, ua, ub, w, K, K, 0, &o), "q of match 3"), "q not finite");
        expect(refused(chk(3, rp, ua, ub, q, k, K, 0, &o), "K_a of pair 1 is not finite"), "K_a not finite");
        expect(refused(chk(3, rp, ua, ub, q, K, k, 0, &o), "K_b of pair 1 is not finite"), "K_b not finite");
        expect(chk(3, rp, ua, ub, q, K, k, 1, &o).empty(), "a shared K is one matrix");
        srk_relate_options b = o;
        b.inlier_pixels = bad;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, &b), "inlier_pixels"), "tau not finite");
    }
    {
        double w[4], k[27];
        std::memcpy(w, q, sizeof w), std::memcpy(k, K, sizeof k);
        w[3] = -1e-300;
        expect(refused(chk(3, rp, ua, ub, w, K, K, 0, &o), "q of match 3"), "negative q");
        k[18 + 8] = 0.0;
        expect(refused(chk(3, rp, ua, ub, q, k, K, 0, &o), "K_a of pair 2 is singular"), "singular K_a");
        expect(refused(chk(3, rp, ua, ub, q, K, k, 0, &o), "K_b of pair 2 is singular"), "singular K_b");
        srk_relate_options b = o;
        b.hypotheses = 0;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, &b), "hypotheses outside 1..4096"), "no hypotheses");
        b.hypotheses = 4097;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, &b), "hypotheses outside 1..4096"), "too many hypotheses");
        b = o;
        b.inlier_pixels = 0.0;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, &b), "inlier_pixels"), "tau = 0");
        b.inlier_pixels = -1.0;
        expect(refused(chk(3, rp, ua, ub, q, K, K, 0, &b), "inlier_pixels"), "tau < 0");
        // more than 2^22 waves: 2^21 + 1 empty pairs at 65 hypotheses are two waves each
        std::vector<int64_t> many((size_t)(1 << 21) + 2, 0);
        b = o;
        b.hypotheses = 65;
        expect(refused(chk((1 << 21) + 1, many.data(), nullptr, nullptr, nullptr, K, K, 1, &b), "split the batch"), "too many waves");
        b.hypotheses = 64;
        expect(chk((1 << 21) + 1, many.data(), nullptr, nullptr, nullptr, K, K, 1, &b).empty(), "one wave each fits");
    }
    {   // the C entry of the host walk refuses and reports: five matches are too few
        double R[9], T[3], E[9], rel[8];
        uint8_t in[4];
        expect(srk_relate_host_pair(4, ua, ub, q, K, K, 1.0, &o, R, T, E, rel, in) == SRK_RELATE_FEW_POINTS && R[0] == 1.0 && T[0] == 0.0 && E[1] == 0.0 &&
                   std::isnan(rel[0]) && rel[1] == 3.0 && std::isnan(rel[7]),
               "few points through the C entry");
        expect(srk_relate_host_pair(4, ua, ub, q, K, K, 1.0, &o, nullptr, T, E, rel, in) == SRK_E_ARGS, "NULL output");
        expect(srk_relate_host_pair(4, ua, ub, q, K, K, nan, &o, R, T, E, rel, in) == SRK_E_ARGS, "f0 not finite");
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}

std::vector<unsigned char> slurp(const char* path)
{
    std::vector<unsigned char> raw;
    if (std::FILE* f = std::fopen(path, "rb")) {
        std::fseek(f, 0, SEEK_END);
        const long size = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        raw.resize((size_t)size);
        if (size > 0 && std::fread(raw.data(), 1, (size_t)size, f) != (size_t)size) raw.clear();
        std::fclose(f);
    }
    return raw;
}

struct Reader {
    const std::vector<unsigned char>& raw;
    size_t pos = 0;
    bool ok = true;
    template <class V> std::vector<V> take(size_t count)
    {
        std::vector<V> v(count);
        if (pos + count * sizeof(V) > raw.size()) {
            ok = false;
            return v;
        }
        if (count) std::memcpy(v.data(), raw.data() + pos, count * sizeof(V));
        pos += count * sizeof(V);
        return v;
    }
};

template <class V> bool put(std::FILE* f, const std::vector<V>& v) { return v.empty() || std::fwrite(v.data(), sizeof(V), v.size(), f) == v.size(); }

int sampler(const char* out, uint64_t seed, int64_t n, int32_t H)
{
    std::vector<int64_t> r((size_t)H * 6);
    for (int32_t h = 0; h < H; ++h) srk_relate_sample(seed, (uint32_t)h, n, r.data() + 6 * (size_t)h);
    std::FILE* f = std::fopen(out, "wb");
    if (!f) return 2;
    const bool ok = put(f, r);
    return std::fclose(f) == 0 && ok ? 0 : 2;
}

int solve(const char* in, const char* out)
{
    const std::vector<unsigned char> raw = slurp(in);
    Reader rd{ raw };
    const std::vector<int64_t> head = rd.take<int64_t>(1);
    if (!rd.ok || head[0] < 0) return 2;
    const size_t n = (size_t)head[0];
    const double f0 = rd.take<double>(1)[0];
    const std::vector<double> Ka = rd.take<double>(9), Kb = rd.take<double>(9), ua = rd.take<double>(12 * n), ub = rd.take<double>(12 * n);
    if (!rd.ok) return 2;
    double Kai[9], Kbi[9];
    srk_relate_inverse3(Ka.data(), Kai);
    srk_relate_inverse3(Kb.data(), Kbi);
    std::vector<double> E(90 * n, 0.0), rec(SRK_RELATE_HYP * n);
    std::vector<int32_t> roots(n);
    for (size_t i = 0; i < n; ++i)
        roots[i] = srk_relate_host_hypothesis(Kai, Kbi, ua.data() + 12 * i, ub.data() + 12 * i, f0, rec.data() + SRK_RELATE_HYP * i, E.data() + 90 * i);
    std::FILE* f = std::fopen(out, "wb");
    if (!f) return 2;
    const bool ok = put(f, E) && put(f, rec) && put(f, roots);
    return std::fclose(f) == 0 && ok ? 0 : 2;
}

int poses(const char* in, const char* out)
{
    const std::vector<unsigned char> raw = slurp(in);
    Reader rd{ raw };
    const std::vector<int64_t> head = rd.take<int64_t>(1);
    if (!rd.ok || head[0] < 0) return 2;
    const size_t n = (size_t)head[0];
    const std::vector<double> E = rd.take<double>(9 * n);
    if (!rd.ok) return 2;
    std::vector<double> R(36 * n), T(12 * n);
    for (size_t i = 0; i < n; ++i) srk_relate_poses_of(E.data() + 9 * i, R.data() + 36 * i, T.data() + 12 * i);
    std::FILE* f = std::fopen(out, "wb");
    if (!f) return 2;
    const bool ok = put(f, R) && put(f, T);
    return std::fclose(f) == 0 && ok ? 0 : 2;
}

int pairs(const char* in, const char* out)
{
    const std::vector<unsigned char> raw = slurp(in);
    Reader rd{ raw };
    const std::vector<int64_t> head = rd.take<int64_t>(5);
    if (!rd.ok || head[0] < 0 || head[1] < 0 || head[3] < 1 || head[3] > 4096) return 2;
    const size_t n = (size_t)head[0], O = (size_t)head[1];
    const std::vector<double> par = rd.take<double>(2);
    const std::vector<int64_t> row_ptr = rd.take<int64_t>(n + 1);
    const std::vector<double> ua = rd.take<double>(2 * O), ub = rd.take<double>(2 * O);
    const std::vector<double> q = rd.take<double>(head[2] ? O : 0);
    const std::vector<double> Ka = rd.take<double>(9 * n), Kb = rd.take<double>(9 * n);
    if (!rd.ok) return 2;
    srk_relate_options o;
    o.hypotheses = (int32_t)head[3];
    o.seed = (uint64_t)head[4];
    o.inlier_pixels = par[1];
    const std::string why = srk_relate_check((int32_t)n, row_ptr.data(), ua.data(), ub.data(), head[2] ? q.data() : nullptr, Ka.data(), Kb.data(), 0, &o);
    if (!why.empty()) {
        std::fprintf(stderr, "%s\n", why.c_str());
        return 3;
    }
    std::vector<double> R(9 * n), T(3 * n), E(9 * n), related(8 * n), scores, all;
    std::vector<uint32_t> status(n);
    std::vector<uint8_t> inl(O);
    for (size_t i = 0; i < n; ++i) {
        const int64_t o0 = row_ptr[i], o1 = row_ptr[i + 1];
        status[i] = srk_relate_host_pair_cpp(o1 - o0, ua.data() + 2 * o0, ub.data() + 2 * o0, head[2] ? q.data() + o0 : nullptr, Ka.data() + 9 * i,
                                             Kb.data() + 9 * i, par[0], o, R.data() + 9 * i, T.data() + 3 * i, E.data() + 9 * i, related.data() + 8 * i,
                                             inl.data() + o0, &scores);
        all.insert(all.end(), scores.begin(), scores.end());
    }
    std::FILE* f = std::fopen(out, "wb");
    if (!f) return 2;
    const bool ok = put(f, R) && put(f, T) && put(f, E) && put(f, related) && put(f, all) && put(f, status) && put(f, inl);
    return std::fclose(f) == 0 && ok ? 0 : 2;
}
} // namespace

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "unit") return unit();
    if (mode == "sampler" && argc == 6)
        return sampler(argv[2], std::strtoull(argv[3], nullptr, 10), std::strtoll(argv[4], nullptr, 10), (int32_t)std::strtol(argv[5], nullptr, 10));
    if (mode == "solve" && argc == 4) return solve(argv[2], argv[3]);
    if (mode == "poses" && argc == 4) return poses(argv[2], argv[3]);
    if (mode == "pairs" && argc == 4) return pairs(argv[2], argv[3]);
    std::fprintf(stderr, "usage: test_relate_host unit | sampler OUT SEED N H | solve IN OUT | poses IN OUT | pairs IN OUT\n");
    return 2;
}
