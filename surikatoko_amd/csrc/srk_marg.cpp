// srk_marg.cpp -- the host arithmetic of the marginalisation priors (srk_marg.hpp).  No HIP header: built with the host compiler
// alone by tests/cpp/test_marg_plan.cpp, and shared by both libraries as srk_factors.o is.
#include "srk_marg.hpp"
#include "srk_geom.hpp"

#include <algorithm>
#include <cmath>

// ------------------------------------------------------------------ the plan

std::string srk_marg_plan(const SrkMargScene& sc, int32_t nd, const int32_t* drop, int64_t np, const int64_t* points, SrkMargPlan& plan)
{
    const char* who = "marginalization: ";
    plan = SrkMargPlan{};
    if (sc.constant_blocks) return std::string(who) + "not available with constant blocks";
    if (sc.intrinsic_groups) return std::string(who) + "not available with intrinsic groups";
    if (sc.multi_rank) return std::string(who) + "not available with more than one rank";
    if (nd < 0 || np < 0 || (nd > 0 && !drop) || (np > 0 && !points)) return std::string(who) + "a negative count, or a NULL list with a positive count";
    if (nd == 0 && np == 0) return std::string(who) + "nothing to marginalise: both lists are empty";
    if (nd > SRK_MARG_MAX_DROP_HOST) return std::string(who) + "at most " + std::to_string(SRK_MARG_MAX_DROP_HOST) + " frames can be dropped by one call";
    for (int32_t i = 0; i < nd; ++i) {
        if (drop[i] < 0 || drop[i] >= sc.M) return std::string(who) + "a frame index lies beyond the scene";
        if (i > 0 && drop[i] <= drop[i - 1]) return std::string(who) + "the frames must be strictly ascending";
    }
    for (int64_t i = 0; i < np; ++i) {
        if (points[i] < 0 || points[i] >= sc.N) return std::string(who) + "a landmark index lies beyond the scene";
        if (i > 0 && points[i] <= points[i - 1]) return std::string(who) + "the landmarks must be strictly ascending";
    }
    const auto f_int = [&](int32_t j) { return sc.frame_int ? sc.frame_int[j] : j; };
    const auto f_user = [&](int32_t j) { return sc.frame_user ? sc.frame_user[j] : j; };
    std::vector<char> in_d((size_t)sc.M, 0), in_p((size_t)sc.N, 0), touched((size_t)sc.M, 0);
    for (int32_t i = 0; i < nd; ++i) in_d[(size_t)f_int(drop[i])] = 1;
    {
        std::vector<char> p_user((size_t)sc.N, 0);
        for (int64_t i = 0; i < np; ++i) p_user[(size_t)points[i]] = 1;
        for (int64_t i = 0; i < sc.N; ++i) in_p[(size_t)i] = p_user[(size_t)sc.perm[i]];
    }
    const auto weighted = [&](int64_t o) { return !sc.q || sc.q[o] > 0; };
    // a weighted observation in a dropped frame whose landmark stays would leave a prior on that landmark
    for (int64_t i = 0; i < sc.N; ++i) {
        if (in_p[(size_t)i]) continue;
        for (int64_t o = sc.row_ptr[i]; o < sc.row_ptr[i + 1]; ++o)
            if (in_d[(size_t)sc.obs_frame[o]] && weighted(o))
                return std::string(who) + "landmark " + std::to_string(sc.perm[i]) + " is observed from the dropped frame " +
                       std::to_string(f_user(sc.obs_frame[o])) + " and is not marginalised (add it to the landmarks, or switch the observation off)";
    }
    // the selected landmarks and the frames their weighted observations touch
    for (int64_t i = 0; i < sc.N; ++i) {
        if (!in_p[(size_t)i]) continue;
        int64_t nw = 0;
        for (int64_t o = sc.row_ptr[i]; o < sc.row_ptr[i + 1]; ++o) nw += weighted(o) ? 1 : 0;
        if (nw < 2) { ++plan.n_single; continue; }
        plan.lm.push_back((int32_t)i);
        plan.lm_row.push_back(plan.n_rows);
        plan.lm_stage.push_back(plan.n_stage);
        plan.n_rows += SRK_MARG_ROWS;
        plan.n_stage += sc.row_ptr[i + 1] - sc.row_ptr[i];
        const int32_t* pe = sc.pt_prior + sc.n_pt_priors;
        const int32_t* at = sc.n_pt_priors > 0 ? std::lower_bound(sc.pt_prior, pe, (int32_t)i) : pe;
        plan.lm_prior.push_back(at != pe && *at == (int32_t)i ? (int32_t)(at - sc.pt_prior) : -1);
        for (int64_t o = sc.row_ptr[i]; o < sc.row_ptr[i + 1]; ++o)
            if (weighted(o)) touched[(size_t)sc.obs_frame[o]] = 1;
    }
    for (int32_t f = 0; f < sc.n_rp; ++f)
        if (in_d[(size_t)sc.rp_a[f]] || in_d[(size_t)sc.rp_b[f]]) {
            plan.factors.push_back(f);
            touched[(size_t)sc.rp_a[f]] = touched[(size_t)sc.rp_b[f]] = 1;
        }
    for (int32_t g = 0; g < sc.n_sets; ++g) {
        bool hit = false;
        for (int32_t s = sc.set_ptr[g]; s < sc.set_ptr[g + 1]; ++s) hit = hit || in_d[(size_t)sc.set_frame[s]];
        if (!hit) continue;
        plan.sets.push_back(g);
        for (int32_t s = sc.set_ptr[g]; s < sc.set_ptr[g + 1]; ++s) touched[(size_t)sc.set_frame[s]] = 1;
    }
    for (int32_t p = 0; p < sc.n_fr_priors; ++p)
        if (in_d[(size_t)sc.fr_prior[p]]) plan.fr_priors.push_back(p);
    for (int32_t j = 0; j < sc.M; ++j) // the caller's numbering, ascending
        if (touched[(size_t)f_int(j)] && !in_d[(size_t)f_int(j)]) plan.kept.push_back(j);
    if ((int64_t)plan.kept.size() > SRK_MARG_MAX_KEPT_HOST) {
        const std::string e = std::string(who) + std::to_string(plan.kept.size()) + " kept frames, at most " +
                              std::to_string(SRK_MARG_MAX_KEPT_HOST) + " (marginalise fewer landmarks, or switch long tracks' observations off)";
        plan = SrkMargPlan{};
        return e;
    }
    plan.d = nd;
    plan.k = (int32_t)plan.kept.size();
    plan.frame_slot.assign((size_t)sc.M, -1);
    for (int32_t i = 0; i < nd; ++i) plan.slot_frame.push_back(f_int(drop[i]));
    for (int32_t j : plan.kept) plan.slot_frame.push_back(f_int(j));
    for (size_t s = 0; s < plan.slot_frame.size(); ++s) plan.frame_slot[(size_t)plan.slot_frame[s]] = (int32_t)s;
    // per slot the staging rows of its weighted observations, landmarks ascending
    const int32_t ns = plan.d + plan.k;
    std::vector<int32_t> cnt((size_t)ns + 1, 0);
    for (size_t l = 0; l < plan.lm.size(); ++l) {
        const int64_t i = plan.lm[l];
        for (int64_t o = sc.row_ptr[i]; o < sc.row_ptr[i + 1]; ++o)
            if (weighted(o)) ++cnt[(size_t)plan.frame_slot[(size_t)sc.obs_frame[o]] + 1];
    }
    plan.slot_ptr.assign((size_t)ns + 1, 0);
    for (int32_t s = 0; s < ns; ++s) plan.slot_ptr[(size_t)s + 1] = plan.slot_ptr[(size_t)s] + cnt[(size_t)s + 1];
    plan.slot_ent.assign((size_t)plan.slot_ptr[(size_t)ns], 0);
    std::vector<int32_t> fill(plan.slot_ptr.begin(), plan.slot_ptr.end() - 1);
    for (size_t l = 0; l < plan.lm.size(); ++l) {
        const int64_t i = plan.lm[l];
        for (int64_t o = sc.row_ptr[i]; o < sc.row_ptr[i + 1]; ++o)
            if (weighted(o)) plan.slot_ent[(size_t)fill[(size_t)plan.frame_slot[(size_t)sc.obs_frame[o]]]++] = plan.lm_stage[l] + (o - sc.row_ptr[i]);
    }
    return {};
}

// ------------------------------------------------------------------ the dense elimination

// Symmetric elimination of W [n][n] with the right-hand side y over the variables [v0, v1), largest remaining diagonal entry first.
// A pivot <= tol ends it.  order receives the pivots taken; a pivot's row is left as it was when it was taken (the row of the
// upper triangular factor), the rows of the variables not yet taken -- inside and outside [v0, v1) -- carry the Schur complement.
static void eliminate(std::vector<double>& W, std::vector<double>& y, int64_t n, int64_t v0, int64_t v1, double tol, std::vector<int64_t>& order)
{
    std::vector<char> done((size_t)n, 0);
    order.clear();
    for (int64_t t = v0; t < v1; ++t) {
        int64_t p = -1;
        for (int64_t i = v0; i < v1; ++i)
            if (!done[(size_t)i] && (p < 0 || W[(n + 1) * i] > W[(n + 1) * p])) p = i;
        if (p < 0 || !(W[(n + 1) * p] > tol)) return;
        done[(size_t)p] = 1;
        order.push_back(p);
        const double ip = 1.0 / W[(n + 1) * p];
        for (int64_t i = 0; i < n; ++i) {
            if (done[(size_t)i]) continue;
            const double f = W[n * i + p] * ip;
            if (f == 0) continue;
            for (int64_t j = 0; j < n; ++j)
                if (!done[(size_t)j]) W[n * i + j] -= f * W[n * p + j];
            y[(size_t)i] -= f * y[(size_t)p];
        }
    }
}

int srk_marg_dense(const double* A, const double* b, int32_t d, int32_t k, double* Lam, double* eta, double* m, double* defect)
{
    const int64_t nd = 6 * (int64_t)d, nk = 6 * (int64_t)k, n = nd + nk;
    std::vector<double> W(A, A + n * n), y(b, b + n);
    std::vector<int64_t> order;
    if (nd > 0) {
        double mx = 0;
        for (int64_t i = 0; i < nd; ++i)
            for (int64_t j = 0; j < nd; ++j) mx = std::max(mx, std::fabs(A[n * i + j]));
        eliminate(W, y, n, 0, nd, 1e-12 * mx, order);
        if ((int64_t)order.size() < nd) return 1;
    }
    std::vector<double> L((size_t)(nk * nk)), e((size_t)nk);
    for (int64_t i = 0; i < nk; ++i) {
        e[(size_t)i] = y[(size_t)(nd + i)];
        for (int64_t j = 0; j < nk; ++j) L[(size_t)(nk * i + j)] = 0.5 * (W[n * (nd + i) + nd + j] + W[n * (nd + j) + nd + i]);
    }
    for (double v : L)
        if (!std::isfinite(v)) return 1;
    // the basic solution of Lam m = -eta
    std::vector<double> Wm(L), ym((size_t)nk), x((size_t)nk, 0.0);
    for (int64_t i = 0; i < nk; ++i) ym[(size_t)i] = -e[(size_t)i];
    double ml = 0;
    for (double v : L) ml = std::max(ml, std::fabs(v));
    eliminate(Wm, ym, nk, 0, nk, 1e-12 * ml, order);
    for (int64_t t = (int64_t)order.size() - 1; t >= 0; --t) {
        const int64_t p = order[(size_t)t];
        double v = ym[(size_t)p];
        for (int64_t s = t + 1; s < (int64_t)order.size(); ++s) v -= Wm[(size_t)(nk * p + order[(size_t)s])] * x[(size_t)order[(size_t)s]];
        x[(size_t)p] = v / Wm[(size_t)((nk + 1) * p)];
    }
    double rn = 0, en = 0;
    for (int64_t i = 0; i < nk; ++i) {
        double r = e[(size_t)i];
        for (int64_t j = 0; j < nk; ++j) r += L[(size_t)(nk * i + j)] * x[(size_t)j];
        rn = std::max(rn, std::fabs(r));
        en = std::max(en, std::fabs(e[(size_t)i]));
    }
    if (Lam) std::copy(L.begin(), L.end(), Lam);
    if (eta) std::copy(e.begin(), e.end(), eta);
    if (m) std::copy(x.begin(), x.end(), m);
    if (defect) *defect = en > 0 ? rn / en : 0.0;
    return 0;
}

// ------------------------------------------------------------------ back into the caller's coordinates

void srk_marg_revert(const srk_ba_normalizer& nrm, int32_t k, double* lin_R, double* lin_C, double* Lam, double* eta, double* m)
{
    const double s = nrm.world_scale, is = 1.0 / s;
    const double* R0 = nrm.R0;
    double R0t[9];
    srk::mat3_tr(R0, R0t);
    const int64_t n = 6 * (int64_t)k;
    for (int32_t q = 0; q < k; ++q) {
        if (lin_R) srk::mat3_mul(lin_R + 9 * q, R0, lin_R + 9 * q);
        if (lin_C) {
            double c[3] = { lin_C[3 * q] * is - nrm.T0[0], lin_C[3 * q + 1] * is - nrm.T0[1], lin_C[3 * q + 2] * is - nrm.T0[2] };
            srk::mat3_vec(R0t, c, lin_C + 3 * q);
        }
        if (eta) { // D^T eta_n: s R0^T on the translation part, R0^T on the rotation part
            srk::mat3_vec(R0t, eta + 6 * q, eta + 6 * q);
            for (int e = 0; e < 3; ++e) eta[6 * q + e] *= s;
            srk::mat3_vec(R0t, eta + 6 * q + 3, eta + 6 * q + 3);
        }
        if (m) { // D^-1 m_n: R0^T / s, R0^T
            srk::mat3_vec(R0t, m + 6 * q, m + 6 * q);
            for (int e = 0; e < 3; ++e) m[6 * q + e] *= is;
            srk::mat3_vec(R0t, m + 6 * q + 3, m + 6 * q + 3);
        }
    }
    if (!Lam) return;
    for (int64_t bi = 0; bi < 2 * (int64_t)k; ++bi) // 3 x 3 blocks: even = translation, odd = rotation; block = f R0^T B R0
        for (int64_t bj = 0; bj < 2 * (int64_t)k; ++bj) {
            double B[9], T[9], U[9];
            for (int a = 0; a < 3; ++a)
                for (int c = 0; c < 3; ++c) B[3 * a + c] = Lam[(3 * bi + a) * n + 3 * bj + c];
            srk::mat3_mul(R0t, B, T);
            srk::mat3_mul(T, R0, U);
            const double f = ((bi & 1) ? 1.0 : s) * ((bj & 1) ? 1.0 : s);
            for (int a = 0; a < 3; ++a)
                for (int c = 0; c < 3; ++c) Lam[(3 * bi + a) * n + 3 * bj + c] = f * U[3 * a + c];
        }
    for (int64_t r = 0; r < n; ++r)
        for (int64_t c = r + 1; c < n; ++c) Lam[r * n + c] = Lam[c * n + r] = 0.5 * (Lam[r * n + c] + Lam[c * n + r]);
}

// ------------------------------------------------------------------ the host-only entry points of include/srk_ba.h

extern "C" {

int srk_ba_marginalize_dense(const double* A, const double* b, int32_t d, int32_t k, double* info, double* eta, double* mean, double* defect)
{
    if (!A || !b || d < 0 || k < 0 || d + k < 1 || d > SRK_MARG_MAX_DROP_HOST || k > SRK_MARG_MAX_KEPT_HOST) return SRK_E_ARGS;
    const int64_t n = 6 * (int64_t)(d + k);
    for (int64_t e = 0; e < n * n; ++e)
        if (!std::isfinite(A[e])) return SRK_E_ARGS;
    for (int64_t e = 0; e < n; ++e)
        if (!std::isfinite(b[e])) return SRK_E_ARGS;
    return srk_marg_dense(A, b, d, k, info, eta, mean, defect);
}

int srk_ba_revert_marginalization_prior(const srk_ba_normalizer* nrm, int32_t k, double* lin_R, double* lin_C, double* info, double* eta,
                                        double* mean)
{
    if (!nrm || k < 0 || !(nrm->world_scale > 0) || !std::isfinite(nrm->world_scale)) return SRK_E_ARGS;
    srk_marg_revert(*nrm, k, lin_R, lin_C, info, eta, mean);
    return SRK_OK;
}

} // extern "C"
