// The scene planner alone (surikatoko_amd/csrc/srk_plan.cpp: no HIP, no device): reads the case files
// tests/scene_plan_cases.py writes and prints, per case, every scalar decision ("s name value") and for every table its
// element count and the 64-bit FNV-1a digest of its bytes ("t name count digest").  A table the upload would not copy to the
// device is printed as empty.  "x" lines are checks made here.  tests/test_scene_plan_cpu.py compares with the parent commit's.
#include "../../surikatoko_amd/csrc/srk_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>

static uint64_t fnv1a(const void* p, size_t n)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}
template <typename T> static void table(const char* name, bool on, const std::vector<T>& v)
{
    const size_t count = on ? v.size() : 0;
    printf("t %s %zu %016llx\n", name, count, (unsigned long long)fnv1a(v.data(), count * sizeof(T)));
}
static void scalar(const char* name, long long v) { printf("s %s %lld\n", name, v); }

template <typename T> static bool read_vec(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int run_case(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 1; }
    std::vector<int64_t> head, row_ptr;
    std::vector<int32_t> obs_frame, order;
    std::vector<double> obs_uv, pts, camR, camT, K;
    bool ok = read_vec(f, head, 12);
    const int64_t N = ok ? head[0] : 0, M = ok ? head[1] : 0, O = ok ? head[2] : 0;
    ok = ok && read_vec(f, row_ptr, (size_t)N + 1) && read_vec(f, obs_frame, (size_t)O) && read_vec(f, obs_uv, (size_t)(2 * O)) &&
         read_vec(f, pts, (size_t)(3 * N)) && read_vec(f, camR, (size_t)(9 * M)) && read_vec(f, camT, (size_t)(3 * M)) &&
         read_vec(f, K, (size_t)(9 * M)) && (!head[8] || read_vec(f, order, (size_t)M));
    fclose(f);
    if (!ok || row_ptr[(size_t)N] != O) { fprintf(stderr, "%s: short or inconsistent case file\n", path); return 1; }

    const SrkSceneIn in{ N, (int32_t)M, row_ptr.data(), obs_frame.data(), obs_uv.data(), pts.data(), camR.data(), camT.data(), K.data() };
    SrkPlanOptions opt;
    opt.fixed_k = head[3] != 0;
    opt.deterministic = head[4] != 0;
    opt.schur_fp32 = head[5] != 0;
    opt.jac_mode = (int)head[6];
    opt.frame_order_mode = (int)head[7];
    opt.frame_order = &order;
    opt.multi_rank = head[9] != 0;
    opt.cus = 256; // what an MI355X reports, and what the parent's planning code assumed when no device answered
    SrkScenePlan p;
    srk_plan_scene(in, opt, p, nullptr);

    const char* base = strrchr(path, '/');
    printf("case %s\n", base ? base + 1 : path);
    scalar("g0", p.g0); scalar("g1", p.g1); scalar("frame_order_supplied", p.frame_order_supplied); scalar("max_frame_obs", p.max_frame_obs);
    scalar("n_cal_list", p.n_cal_list); scalar("n_long_items", p.n_long_items); scalar("n_long_runs", p.n_long_runs);
    scalar("n_groups", p.n_groups); scalar("n_groups_wide", p.n_groups_wide); scalar("n_groups_mid", p.n_groups_mid); scalar("n_generic", p.n_generic);
    scalar("n_mm_uniform", p.n_mm_uniform); scalar("n_mm_ragged", p.n_mm_ragged);
    scalar("jac_fused", p.jac_fused); scalar("jac_runs", p.jac_runs); scalar("jac_runs_masked", p.jac_runs_masked); scalar("jr_own_runs", p.jr_own_runs);
    scalar("jr_tasks", p.jr_tasks); scalar("jr_min_nf", p.jr_min_nf); scalar("det_active", p.det_active); scalar("ds_n_pairs", p.ds_n_pairs);
    scalar("long_fb", p.long_fb);
    table("perm", true, p.perm); table("row_ptr_user", true, p.row_ptr_user); table("frame_int", true, p.frame_int); table("frame_user", true, p.frame_user);
    table("obs_rank", true, p.obs_rank); table("fobs_of", true, p.fobs_of); table("min_cv", true, p.min_cv);
    table("pts", true, p.pts); table("camR", true, p.camR); table("camT", true, p.camT); table("K", true, p.K);
    table("row_ptr", true, p.row_ptr_int); table("obs_frame", true, p.obs_frame); table("obs_pt", true, p.obs_pt); table("obs_uv", true, p.obs_uv);
    table("col_ptr", true, p.col_ptr); table("fobs_pt", true, p.fobs_pt); table("fobs_uv", true, p.fobs_uv); table("wg_jmin", true, p.wg_jmin);
    table("grp_first", true, p.grp_first); table("grp_count", true, p.grp_count); table("grp_nf", true, p.grp_nf); table("grp_frames", true, p.grp_frames);
    table("obs_slot", true, p.obs_slot); table("pt_mask", true, p.pt_mask); table("gen_list", true, p.gen_list); table("cal_list", true, p.cal_list);
    table("lg_item", true, p.lg_item); table("lg_np", true, p.lg_np); table("lg_nf", true, p.lg_nf); table("lg_pts", true, p.lg_pts);
    table("lg_frames", true, p.lg_frames); table("lg_obs_off", true, p.lg_obs_off); table("lg_obs", true, p.lg_obs);
    table("jr_first", p.jac_runs, p.jr_first); table("jr_count", p.jac_runs, p.jr_count); table("jr_jmin", p.jac_runs, p.jr_jmin);
    table("jr_group", p.jac_runs && p.jac_runs_masked, p.jr_group);
    table("jd_nf", p.jr_own_runs, p.jd_nf); table("jd_frames", p.jr_own_runs, p.jd_frames); table("jd_mask", p.jr_own_runs, p.jd_mask);
    table("dj_ptr", p.det_active, p.dj_ptr); table("dj_ent", p.det_active, p.dj_ent); table("ds_pair_ptr", p.det_active, p.ds_pair_ptr);
    table("ds_pair_fa", p.det_active, p.ds_pair_fa); table("ds_pair_fb", p.det_active, p.ds_pair_fb); table("ds_pair_ent", p.det_active, p.ds_pair_ent);
    table("ds_f_ptr", p.det_active, p.ds_f_ptr); table("ds_f_ent", p.det_active, p.ds_f_ent);

    printf("x min_cv_max %d\n", p.min_cv.empty() ? 0 : *std::max_element(p.min_cv.begin(), p.min_cv.end()));
    if (head[10]) { // the landmark order against ONE std::stable_sort with the planner's comparator (the frames keep their order here)
        std::vector<int64_t> one((size_t)N);
        std::iota(one.begin(), one.end(), (int64_t)0);
        std::stable_sort(one.begin(), one.end(), [&](int64_t x, int64_t y) {
            const int64_t ox = row_ptr[x], oy = row_ptr[y], nx = row_ptr[x + 1] - ox, ny = row_ptr[y + 1] - oy;
            if (nx == 0 || ny == 0) return nx < ny;
            if (obs_frame[ox] != obs_frame[oy]) return obs_frame[ox] < obs_frame[oy];
            if (nx != ny) return nx < ny;
            for (int64_t k = 1; k < nx; ++k)
                if (obs_frame[ox + k] != obs_frame[oy + k]) return obs_frame[ox + k] < obs_frame[oy + k];
            return false;
        });
        printf("x perm_is_stable_sort %d\n", p.frame_int.empty() && one == p.perm ? 1 : 0);
    }
    return 0;
}

int main(int argc, char** argv)
{
    for (int a = 1; a < argc; ++a)
        if (run_case(argv[a])) return 1;
    return 0;
}
