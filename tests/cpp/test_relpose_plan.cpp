// The planner with relative-pose pairs, host only (tests/test_relpose_cpu.py builds this with srk_plan.cpp alone).
// usage: test_relpose_plan M window mode [a b]...   -- a banded scene of M frames (four landmarks start at every frame and are
// seen by `window` consecutive frames), frame reordering mode, pairs in the caller's numbering.  Prints min_cv (internal
// numbering), whether the frames were renumbered, the internal indices of the pairs' frames and a digest of every other table.
#include "../../surikatoko_amd/csrc/srk_plan.hpp"

#include <cstdio>
#include <cstdlib>

static uint64_t fnv(uint64_t h, const void* p, size_t n)
{
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}
template <typename T> static uint64_t fnv(uint64_t h, const std::vector<T>& v)
{
    const uint64_t n = v.size();
    h = fnv(h, &n, sizeof n);
    return v.empty() ? h : fnv(h, v.data(), v.size() * sizeof(T));
}

int main(int argc, char** argv)
{
    if (argc < 4 || (argc - 4) % 2) return 2;
    const int32_t M = atoi(argv[1]), window = atoi(argv[2]);
    const int mode = atoi(argv[3]);
    std::vector<int32_t> ra, rb;
    for (int i = 4; i + 1 < argc; i += 2) { ra.push_back(atoi(argv[i])); rb.push_back(atoi(argv[i + 1])); }
    std::vector<int64_t> row_ptr(1, 0);
    std::vector<int32_t> obs_frame;
    for (int32_t j = 0; j < M; ++j)
        for (int r = 0; r < 4; ++r) {
            for (int32_t f = j; f < j + window && f < M; ++f) obs_frame.push_back(f);
            row_ptr.push_back((int64_t)obs_frame.size());
        }
    const int64_t N = (int64_t)row_ptr.size() - 1;
    std::vector<double> uv(2 * obs_frame.size(), 0.0), pts((size_t)(3 * N), 0.0), R(9 * (size_t)M, 0.0), T(3 * (size_t)M, 0.0), K(9 * (size_t)M, 0.0);
    SrkPlanOptions opt;
    opt.frame_order_mode = mode;
    opt.rel_a = ra.data();
    opt.rel_b = rb.data();
    opt.n_rel = (int64_t)ra.size();
    SrkScenePlan p;
    srk_plan_scene({ N, M, row_ptr.data(), obs_frame.data(), uv.data(), pts.data(), R.data(), T.data(), K.data() }, opt, p, nullptr);
    printf("min_cv");
    for (int32_t v : p.min_cv) printf(" %d", v);
    printf("\nrenumbered %d\npairs", p.frame_int.empty() ? 0 : 1);
    for (size_t k = 0; k < ra.size(); ++k)
        printf(" %d %d", p.frame_int.empty() ? ra[k] : p.frame_int[(size_t)ra[k]], p.frame_int.empty() ? rb[k] : p.frame_int[(size_t)rb[k]]);
    uint64_t h = 1469598103934665603ull;
    h = fnv(h, p.perm); h = fnv(h, p.row_ptr_int); h = fnv(h, p.obs_frame); h = fnv(h, p.obs_pt); h = fnv(h, p.frame_int);
    h = fnv(h, p.grp_first); h = fnv(h, p.grp_count); h = fnv(h, p.grp_nf); h = fnv(h, p.grp_frames); h = fnv(h, p.obs_slot);
    h = fnv(h, p.pt_mask); h = fnv(h, p.jr_first); h = fnv(h, p.jr_count); h = fnv(h, p.jr_jmin); h = fnv(h, p.jr_group);
    h = fnv(h, p.wg_jmin); h = fnv(h, p.col_ptr); h = fnv(h, p.lg_item); h = fnv(h, p.gen_list);
    const int64_t sc[] = { p.n_groups, p.n_groups_wide, p.n_groups_mid, p.n_generic, p.n_long_items, p.jac_fused, p.jac_runs, p.jac_runs_masked, p.jr_tasks };
    h = fnv(h, sc, sizeof sc);
    printf("\ndigest %016llx\n", (unsigned long long)h);
    return 0;
}
