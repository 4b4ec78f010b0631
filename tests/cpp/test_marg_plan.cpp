// test_marg_plan.cpp -- the host half of the marginalisation priors (surikatoko_amd/csrc/srk_marg.cpp) and the host terms of
// srk_factors.cpp without a GPU, driven by tests/test_marginal_cpu.py.  Built with the host compiler alone:
//   c++ -std=c++17 tests/cpp/test_marg_plan.cpp surikatoko_amd/csrc/srk_marg.cpp surikatoko_amd/csrc/srk_factors.cpp surikatoko_amd/csrc/srk_plan.cpp
// Usage: test_marg_plan plan|relpose|jprior FILE -- FILE holds whitespace-separated tokens (integers, doubles as C hex floats);
// the answer goes to stdout in the same form.
#include "../../surikatoko_amd/csrc/srk_factors.hpp"
#include "../../surikatoko_amd/csrc/srk_marg.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

namespace {
struct Reader {
    std::ifstream f;
    explicit Reader(const char* path) : f(path) {}
    int64_t i()
    {
        std::string t;
        if (!(f >> t)) { std::fprintf(stderr, "short file\n"); std::exit(2); }
        return std::strtoll(t.c_str(), nullptr, 10);
    }
    double d()
    {
        std::string t;
        if (!(f >> t)) { std::fprintf(stderr, "short file\n"); std::exit(2); }
        return std::strtod(t.c_str(), nullptr);
    }
    template <typename T> std::vector<T> ints()
    {
        std::vector<T> v((size_t)i());
        for (T& x : v) x = (T)i();
        return v;
    }
    std::vector<double> doubles()
    {
        std::vector<double> v((size_t)i());
        for (double& x : v) x = d();
        return v;
    }
};
template <typename T> void put(const char* name, const std::vector<T>& v)
{
    std::printf("%s", name);
    for (const T& x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}
void put(const char* name, const std::vector<double>& v)
{
    std::printf("%s", name);
    for (double x : v) std::printf(" %a", x);
    std::printf("\n");
}

int plan(const char* path)
{
    Reader r(path);
    SrkMargScene sc;
    sc.N = r.i();
    sc.M = (int32_t)r.i();
    const auto row_ptr = r.ints<int64_t>();
    const auto obs_frame = r.ints<int32_t>();
    const auto q = r.doubles();
    const auto perm = r.ints<int64_t>();
    const auto frame_int = r.ints<int32_t>();
    const auto pt_prior = r.ints<int32_t>();
    const auto fr_prior = r.ints<int32_t>();
    const auto rp_a = r.ints<int32_t>();
    const auto rp_b = r.ints<int32_t>();
    const auto set_ptr = r.ints<int32_t>();
    const auto set_frame = r.ints<int32_t>();
    sc.constant_blocks = r.i() != 0;
    sc.intrinsic_groups = r.i() != 0;
    sc.multi_rank = r.i() != 0;
    const auto drop = r.ints<int32_t>();
    const auto points = r.ints<int64_t>();
    std::vector<int32_t> frame_user(frame_int.size());
    for (size_t j = 0; j < frame_int.size(); ++j) frame_user[(size_t)frame_int[j]] = (int32_t)j;
    sc.row_ptr = row_ptr.data();
    sc.obs_frame = obs_frame.data();
    sc.q = q.empty() ? nullptr : q.data();
    sc.perm = perm.data();
    sc.frame_int = frame_int.empty() ? nullptr : frame_int.data();
    sc.frame_user = frame_int.empty() ? nullptr : frame_user.data();
    sc.n_pt_priors = (int64_t)pt_prior.size();
    sc.pt_prior = pt_prior.data();
    sc.n_fr_priors = (int32_t)fr_prior.size();
    sc.fr_prior = fr_prior.data();
    sc.n_rp = (int32_t)rp_a.size();
    sc.rp_a = rp_a.data();
    sc.rp_b = rp_b.data();
    sc.n_sets = set_ptr.empty() ? 0 : (int32_t)set_ptr.size() - 1;
    sc.set_ptr = set_ptr.data();
    sc.set_frame = set_frame.data();
    SrkMargPlan p;
    const std::string why = srk_marg_plan(sc, (int32_t)drop.size(), drop.data(), (int64_t)points.size(), points.data(), p);
    if (!why.empty()) {
        std::printf("refused %s\n", why.c_str());
        return 0;
    }
    std::printf("ok %d %d %d %lld %lld %lld\n", p.d, p.k, p.ldz(), (long long)p.n_rows, (long long)p.n_stage, (long long)p.n_single);
    put("kept", p.kept);
    put("slot_frame", p.slot_frame);
    put("frame_slot", p.frame_slot);
    put("lm", p.lm);
    put("lm_row", p.lm_row);
    put("lm_stage", p.lm_stage);
    put("lm_prior", p.lm_prior);
    put("slot_ptr", p.slot_ptr);
    put("slot_ent", p.slot_ent);
    put("fr_priors", p.fr_priors);
    put("factors", p.factors);
    put("sets", p.sets);
    return 0;
}

int relpose(const char* path)
{
    Reader r(path);
    const int64_t n = r.i();
    for (int64_t c = 0; c < n; ++c) {
        const auto Ra = r.doubles(), Ta = r.doubles(), Rb = r.doubles(), Tb = r.doubles(), Z = r.doubles(), z = r.doubles(), L = r.doubles();
        std::vector<double> H(144), g(12);
        srk_relpose_terms(Ra.data(), Ta.data(), Rb.data(), Tb.data(), Z.data(), z.data(), L.data(), H.data(), g.data());
        put("H", H);
        put("g", g);
    }
    return 0;
}

int jprior(const char* path)
{
    Reader r(path);
    const int64_t n = r.i();
    for (int64_t c = 0; c < n; ++c) {
        const int32_t k = (int32_t)r.i();
        const auto R = r.doubles(), T = r.doubles(), lin = r.doubles(), mean = r.doubles(), L = r.doubles();
        std::vector<double> H((size_t)(36 * k * k)), g((size_t)(6 * k));
        srk_jprior_terms(k, R.data(), T.data(), lin.data(), mean.data(), L.data(), H.data(), g.data());
        put("H", H);
        put("g", g);
    }
    return 0;
}
} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: test_marg_plan plan|relpose|jprior FILE\n");
        return 2;
    }
    const std::string what = argv[1];
    if (what == "plan") return plan(argv[2]);
    if (what == "relpose") return relpose(argv[2]);
    if (what == "jprior") return jprior(argv[2]);
    return 2;
}
