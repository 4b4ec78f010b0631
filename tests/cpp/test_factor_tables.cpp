// The factor settings alone (surikatoko_amd/csrc/srk_factors.cpp and the scene planner: no HIP, no device): reads the case files
// tests/factor_table_cases.py writes, plans each scene, selects and builds every family's tables and prints, per case, the
// counts ("s name value"), for every table its element count and the 64-bit FNV-1a digest of its bytes ("t name count digest"),
// and the residuals of the case's own scene against its settings ("r name values", hex floats).  A first argument "psd" reads
// 6 x 6 matrices instead and prints the verdict of srk_info_psd on each ("x psd k verdict").
// tests/test_factor_tables_cpu.py compares with the parent commit's.
#include "../../surikatoko_amd/csrc/srk_factors.hpp"

#include <cstdio>
#include <cstring>

static uint64_t fnv1a(const void* p, size_t n)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    return h;
}
template <typename T> static void table(const char* name, const std::vector<T>& v)
{
    printf("t %s %zu %016llx\n", name, v.size(), (unsigned long long)fnv1a(v.data(), v.size() * sizeof(T)));
}
static void scalar(const char* name, long long v) { printf("s %s %lld\n", name, v); }
static void values(const char* name, const std::vector<double>& v)
{
    printf("r %s", name);
    for (double x : v) printf(" %a", x);
    printf("\n");
}
template <typename T> static bool read_vec(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static int run_psd(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 1; }
    std::vector<double> A(36);
    for (int k = 0; fread(A.data(), 8, 36, f) == 36; ++k) printf("x psd %d %d\n", k, srk_info_psd(A.data(), 6) ? 1 : 0);
    fclose(f);
    return 0;
}

static int run_case(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 1; }
    std::vector<int64_t> head, row_ptr;
    std::vector<int32_t> obs_frame;
    std::vector<double> obs_uv, pts, camR, camT, K, nrm_a;
    SrkInfoSetting info;
    SrkConstSetting cst;
    SrkPriorSetting pri;
    SrkRelPoseSetting rp;
    SrkJPriorSetting jp;
    bool ok = read_vec(f, head, 20);
    const int64_t N = ok ? head[0] : 0, M = ok ? head[1] : 0, O = ok ? head[2] : 0;
    ok = ok && read_vec(f, row_ptr, (size_t)N + 1) && read_vec(f, obs_frame, (size_t)O) && read_vec(f, obs_uv, (size_t)(2 * O)) &&
         read_vec(f, pts, (size_t)(3 * N)) && read_vec(f, camR, (size_t)(9 * M)) && read_vec(f, camT, (size_t)(3 * M)) &&
         read_vec(f, K, (size_t)(9 * M)) && read_vec(f, nrm_a, 13) && read_vec(f, info.q, (size_t)head[5]) &&
         read_vec(f, cst.frames, (size_t)head[8]) && read_vec(f, cst.points, (size_t)head[9]) &&
         read_vec(f, pri.pt_idx, (size_t)head[12]) && read_vec(f, pri.pt_pos, (size_t)(3 * head[12])) && read_vec(f, pri.pt_info, (size_t)(6 * head[12])) &&
         read_vec(f, pri.fr_idx, (size_t)head[13]) && read_vec(f, pri.fr_pos, (size_t)(3 * head[13])) && read_vec(f, pri.fr_info, (size_t)(6 * head[13])) &&
         read_vec(f, rp.a, (size_t)head[14]) && read_vec(f, rp.b, (size_t)head[14]) && read_vec(f, rp.R, (size_t)(9 * head[14])) &&
         read_vec(f, rp.t, (size_t)(3 * head[14])) && read_vec(f, rp.info, (size_t)(21 * head[14])) &&
         read_vec(f, jp.ptr, (size_t)head[15] + 1) && read_vec(f, jp.frame, (size_t)head[17]) && read_vec(f, jp.R, (size_t)(9 * head[17])) &&
         read_vec(f, jp.C, (size_t)(3 * head[17])) && read_vec(f, jp.mean, (size_t)(6 * head[17])) && read_vec(f, jp.info, (size_t)head[18]);
    fclose(f);
    if (!ok || row_ptr[(size_t)N] != O) { fprintf(stderr, "%s: short or inconsistent case file\n", path); return 1; }
    cst.set = head[6] != 0;
    cst.keep_gauge = (int)head[7];
    pri.set = head[10] != 0;
    pri.keep_gauge = (int)head[11];
    rp.set = head[14] > 0;
    jp.set = head[15] > 0;
    jp.keep_gauge = (int)head[16];
    if (!jp.set) jp.ptr.clear(); // as the setter leaves a cleared setting
    srk_ba_normalizer nrm;
    std::memcpy(nrm.R0, nrm_a.data(), 72);
    std::memcpy(nrm.T0, nrm_a.data() + 9, 24);
    nrm.world_scale = nrm_a[12];

    const char* base = strrchr(path, '/');
    printf("case %s\n", base ? base + 1 : path);
    // the setters' checks accept what the case files hold
    const char* e = srk_check_prior_values((int64_t)pri.pt_idx.size(), pri.pt_pos.data(), pri.pt_info.data());
    if (!e) e = srk_check_prior_values((int64_t)pri.fr_idx.size(), pri.fr_pos.data(), pri.fr_info.data());
    if (!e) e = srk_check_relpose((int32_t)rp.a.size(), rp.a.data(), rp.b.data(), rp.R.data(), rp.t.data(), rp.info.data());
    if (!e && jp.set) e = srk_check_jprior((int32_t)jp.ptr.size() - 1, jp.ptr.data(), jp.frame.data(), jp.R.data(), jp.C.data(), jp.mean.data(), jp.info.data(), jp.keep_gauge);
    if (e) { fprintf(stderr, "%s: %s\n", path, e); return 1; }

    SrkFactorSelection sel;
    const std::string refused = srk_select_factors(cst, pri, rp, jp, N, (int32_t)M, sel);
    if (!refused.empty()) { fprintf(stderr, "%s: %s\n", path, refused.c_str()); return 1; }
    table("rel_a", sel.rel_a); table("rel_b", sel.rel_b);

    const SrkSceneIn in{ N, (int32_t)M, row_ptr.data(), obs_frame.data(), obs_uv.data(), pts.data(), camR.data(), camT.data(), K.data() };
    SrkPlanOptions opt;
    opt.fixed_k = head[3] != 0;
    opt.frame_order_mode = (int)head[4];
    opt.cus = 256; // what an MI355X reports
    opt.rel_a = sel.rel_a.data();
    opt.rel_b = sel.rel_b.data();
    opt.n_rel = (int64_t)sel.rel_a.size();
    SrkScenePlan plan;
    srk_plan_scene(in, opt, plan, nullptr);
    const int fv = opt.fixed_k ? 6 : 10;
    const SrkFactorDims d{ N, (int32_t)M, O, fv, (fv * M + 255) / 256 * 256 };

    const SrkInfoTables ti = srk_build_information(info, plan, d);
    scalar("info_on", ti.on);
    table("info_q", ti.q); table("info_qf", ti.qf);
    const SrkConstTables tc = srk_build_constant(cst, plan, d);
    scalar("n_cst_pts", (long long)tc.pts.size()); scalar("n_cst_frames", (long long)tc.frames.size());
    table("cst_pts", tc.pts); table("cst_frames", tc.frames); table("cst_frame_int", tc.frame_int);
    const SrkPriorTables tp = srk_build_priors(pri, nrm, plan, d);
    scalar("n_pri_pts", (long long)tp.pt_list.size()); scalar("n_pri_frames", (long long)tp.fr_list.size());
    table("pri_pt_list", tp.pt_list); table("pri_pt_val", tp.pt_val); table("pri_fr_list", tp.fr_list); table("pri_fr_val", tp.fr_val);
    const SrkRelPoseTables tr = srk_build_relpose(rp, sel, nrm, plan, d);
    scalar("n_rp", (long long)tr.fa.size()); scalar("n_rp_frames", (long long)tr.fr_list.size());
    table("rp_fa", tr.fa); table("rp_fb", tr.fb); table("rp_val", tr.val); table("rp_fr_list", tr.fr_list); table("rp_fr_ptr", tr.fr_ptr);
    table("rp_fr_ent", tr.fr_ent); table("rp_tgt", tr.tgt); table("rp_int_a", tr.fa); table("rp_int_b", tr.fb);
    const SrkJPriorTables tj = srk_build_jprior(jp, sel, nrm, plan, d);
    scalar("n_jp", (long long)tj.iptr.size()); scalar("n_jp_pairs", (long long)tj.pslot.size()); scalar("n_jp_frames", (long long)tj.fr_list.size());
    table("jp_ptr", tj.ptr); table("jp_frame", tj.frame); table("jp_lin", tj.lin); table("jp_mean", tj.mean); table("jp_iptr", tj.iptr);
    table("jp_info", tj.info); table("jp_pptr", tj.pptr); table("jp_pslot", tj.pslot); table("jp_tgt", tj.tgt); table("jp_fr_list", tj.fr_list);
    table("jp_fr_ptr", tj.fr_ptr); table("jp_fr_ent", tj.fr_ent); table("jp_pair_a", tj.pair_a); table("jp_pair_b", tj.pair_b);

    // the residuals of the case's own scene (the caller's world) against the settings as an upload would have taken them
    SrkPriorApplied ap;
    SrkRelPoseApplied ar;
    SrkJPriorApplied aj;
    ap.take(pri); ar.take(rp); aj.take(jp);
    if (!ap.is(pri) || !ar.is(rp) || !aj.is(jp)) { fprintf(stderr, "%s: a snapshot differs from its setting\n", path); return 1; }
    std::vector<double> dp(3 * ap.pt_idx.size()), df(3 * ap.fr_idx.size()), er(6 * ar.a.size()), ej(6 * aj.frame.size());
    srk_prior_residuals(ap, pts.data(), camR.data(), camT.data(), dp.data(), df.data());
    srk_relpose_residuals(ar, camR.data(), camT.data(), er.data());
    srk_jprior_residuals(aj, camR.data(), camT.data(), ej.data());
    values("prior_points", dp); values("prior_frames", df); values("relpose", er); values("jprior", ej);
    // a change of information alone does not change a snapshot
    for (double& v : rp.info) v *= 2;
    for (double& v : jp.info) v *= 2;
    for (double& v : pri.pt_info) v *= 2;
    printf("x snapshot_ignores_information %d\n", ap.is(pri) && ar.is(rp) && aj.is(jp) ? 1 : 0);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 2 && !strcmp(argv[1], "psd")) return run_psd(argv[2]);
    for (int a = 1; a < argc; ++a)
        if (run_case(argv[a])) return 1;
    return 0;
}
