// srk_plan.cpp -- the scene planner (srk_plan.hpp): host-only integer bookkeeping between the caller's scene and the device tables.
#include "srk_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <numeric>
#include <thread>
#include <unordered_set>
#include <utility>

bool srk_debug()
{
    static const bool on = getenv("SRK_DEBUG") != nullptr;
    return on;
}

// Internal frame order.  The reference treats the reduced camera system as a dense matrix (bundle-adj-kanatani.cpp:1911), so
// the order of the frames means nothing to it.  Here everything fast depends on covisible frames having NEARBY indices: the
// skyline of the system, its nested dissection (separators one bandwidth wide), the frame windows of the derivative kernels.
// An image sequence in time order has that property; the same frames in any other order (an unordered image set), or a
// sequence that closes a loop (the last frames see the first frames' landmarks), do not -- the solve alone then takes 5x
// longer on the 1000-frame scene (one skyline chain instead of chunks).  So, when the caller's order is far from banded,
// the frames are renumbered by reverse Cuthill-McKee on the covisibility graph (two frames adjacent iff they share a
// landmark), started from a pseudo-peripheral frame: a shuffled sequence gets its band back, a closed loop becomes a band
// of two to three times the width (twice is the optimum for a ring).  Only the numbering changes -- arithmetic per block, gauge (the caller's frames 0 and 1, wherever they
// land: SrkDims::g0, g1) and results are those of the caller's order; every download maps back.
// Returns true and fills to_int[caller's frame] = internal index when renumbering pays.  mode: SrkPlanOptions::frame_order_mode.
// rel_a / rel_b: pairs of frames tied by a relative-pose factor -- edges of the graph like a shared landmark.
bool srk_frame_reorder(int mode, int64_t N, int32_t M, const int64_t* row_ptr, const int32_t* obs_frame, std::vector<int32_t>& to_int,
                       const int32_t* rel_a, const int32_t* rel_b, int64_t n_rel)
{
    if (mode == 0 || M < 3 || M > 16384) return false;
    int64_t bw_nat = 0, lmax = 0;
    for (int64_t i = 0; i < N; ++i) {
        const int64_t k = row_ptr[i + 1] - row_ptr[i];
        if (k < 1) continue;
        lmax = std::max(lmax, k);
        bw_nat = std::max<int64_t>(bw_nat, obs_frame[row_ptr[i + 1] - 1] - obs_frame[row_ptr[i]]); // lists ascend
    }
    for (int64_t k = 0; k < n_rel; ++k) bw_nat = std::max<int64_t>(bw_nat, std::abs(rel_a[k] - rel_b[k]));
    if (mode < 0 && bw_nat <= 2 * lmax) return false; // as banded as tracks of that length allow
    // covisibility graph as a bit matrix (M <= 16384: 32 MB); every distinct frame list once
    const size_t wpr = ((size_t)M + 63) / 64;
    std::vector<uint64_t> adj((size_t)M * wpr, 0);
    std::unordered_set<uint64_t> seen;
    int64_t pair_work = 0;
    const int64_t pair_budget = 400000000; // ~1 s of host time
    for (int64_t i = 0; i < N; ++i) {
        const int64_t k = row_ptr[i + 1] - row_ptr[i];
        if (k < 2) continue;
        const int32_t* f = obs_frame + row_ptr[i];
        uint64_t hsh = 1469598103934665603ull ^ (uint64_t)k;
        for (int64_t a = 0; a < k; ++a) hsh = (hsh ^ (uint64_t)(uint32_t)f[a]) * 1099511628211ull;
        if (!seen.insert(hsh).second) continue; // (a collision only costs ordering quality: the skyline is built from the observations)
        auto link = [&](int32_t u, int32_t v) {
            adj[(size_t)u * wpr + (size_t)(v >> 6)] |= 1ull << (v & 63);
            adj[(size_t)v * wpr + (size_t)(u >> 6)] |= 1ull << (u & 63);
        };
        // all pairs of a list while the work stays bounded (long ragged tracks in an unordered set: ~1e6 distinct lists of
        // ~500 frames would be 1e11 insertions before the first kernel); beyond the budget a list's chain of consecutive
        // frames plus its first-last pair, which keeps the graph connected along every track
        if (pair_work + k * (k - 1) / 2 <= pair_budget) {
            pair_work += k * (k - 1) / 2;
            for (int64_t a = 0; a < k; ++a)
                for (int64_t b = a + 1; b < k; ++b) link(f[a], f[b]);
        } else {
            for (int64_t a = 0; a + 1 < k; ++a) link(f[a], f[a + 1]);
            link(f[0], f[k - 1]);
        }
    }
    for (int64_t k = 0; k < n_rel; ++k) {
        const int32_t u = rel_a[k], v = rel_b[k];
        adj[(size_t)u * wpr + (size_t)(v >> 6)] |= 1ull << (v & 63);
        adj[(size_t)v * wpr + (size_t)(u >> 6)] |= 1ull << (u & 63);
    }
    std::vector<int32_t> deg((size_t)M, 0);
    for (int32_t j = 0; j < M; ++j)
        for (size_t w = 0; w < wpr; ++w) deg[(size_t)j] += __builtin_popcountll(adj[(size_t)j * wpr + w]);
    std::vector<int32_t> order, level((size_t)M), nb;
    std::vector<char> done((size_t)M, 0);
    // breadth-first levels of the component of `root` among the frames not yet numbered; returns the last level's
    // frame of smallest degree and the depth
    std::vector<int32_t> stamp((size_t)M, 0); // visited in THIS search: stamp == bfs_id (no copy of an M-byte array per search)
    int32_t bfs_id = 0;
    auto bfs = [&](int32_t root, std::vector<int32_t>& out, int32_t& depth) -> int32_t {
        out.clear();
        out.push_back(root);
        ++bfs_id;
        struct Vis {
            const std::vector<char>& done;
            std::vector<int32_t>& stamp;
            int32_t id;
            struct Ref {
                Vis& v;
                size_t i;
                operator bool() const { return v.done[i] || v.stamp[i] == v.id; }
                Ref& operator=(int) { v.stamp[i] = v.id; return *this; }
            };
            Ref operator[](size_t i) { return Ref{ *this, i }; }
        } vis{ done, stamp, bfs_id };
        vis[(size_t)root] = 1;
        level[(size_t)root] = 0;
        for (size_t q = 0; q < out.size(); ++q) {
            const int32_t u = out[q];
            nb.clear();
            for (size_t w = 0; w < wpr; ++w)
                for (uint64_t bits = adj[(size_t)u * wpr + w]; bits; bits &= bits - 1) {
                    const int32_t v = (int32_t)(64 * w) + __builtin_ctzll(bits);
                    if (!vis[(size_t)v]) { vis[(size_t)v] = 1; nb.push_back(v); }
                }
            std::sort(nb.begin(), nb.end(), [&](int32_t a, int32_t b) { return deg[(size_t)a] != deg[(size_t)b] ? deg[(size_t)a] < deg[(size_t)b] : a < b; });
            for (int32_t v : nb) { level[(size_t)v] = level[(size_t)u] + 1; out.push_back(v); }
        }
        depth = level[(size_t)out.back()];
        int32_t far = out.back();
        for (size_t q = out.size(); q-- > 0 && level[(size_t)out[q]] == depth;)
            if (deg[(size_t)out[q]] < deg[(size_t)far] || (deg[(size_t)out[q]] == deg[(size_t)far] && out[q] < far)) far = out[q];
        return far;
    };
    std::vector<int32_t> comp;
    for (int32_t start = 0; start < M; ++start) {
        if (done[(size_t)start]) continue;
        if (deg[(size_t)start] == 0) { // a frame nobody shares a landmark with: a component of its own
            done[(size_t)start] = 1;
            order.push_back(start);
            continue;
        }
        int32_t root = start, depth = -1, d2 = 0;
        for (int it = 0; it < 4; ++it) { // George-Liu: walk to a frame of (nearly) greatest eccentricity
            const int32_t far = bfs(root, comp, d2);
            if (d2 <= depth) break;
            depth = d2;
            root = far;
        }
        bfs(root, comp, d2);
        for (int32_t v : comp) { done[(size_t)v] = 1; order.push_back(v); }
    }
    std::reverse(order.begin(), order.end());
    to_int.assign((size_t)M, 0);
    for (int32_t i = 0; i < M; ++i) to_int[(size_t)order[(size_t)i]] = i;
    int64_t bw_new = 0;
    bool differs = false;
    for (int32_t j = 0; j < M; ++j) differs = differs || to_int[(size_t)j] != j;
    for (int64_t i = 0; i < N; ++i) {
        int32_t lo = M, hi = -1;
        for (int64_t o = row_ptr[i]; o < row_ptr[i + 1]; ++o) {
            lo = std::min(lo, to_int[(size_t)obs_frame[o]]);
            hi = std::max(hi, to_int[(size_t)obs_frame[o]]);
        }
        if (hi >= 0) bw_new = std::max<int64_t>(bw_new, hi - lo);
    }
    for (int64_t k = 0; k < n_rel; ++k) bw_new = std::max<int64_t>(bw_new, std::abs(to_int[(size_t)rel_a[k]] - to_int[(size_t)rel_b[k]]));
    if (srk_debug()) fprintf(stderr, "srk_ba frame order: bandwidth %lld frames in the caller's order, %lld after reverse Cuthill-McKee\n", (long long)bw_nat, (long long)bw_new);
    return mode > 0 ? differs : 10 * bw_new <= 7 * bw_nat;
}

namespace {

using Plan = SrkScenePlan;

// CSR by key: each(emit) calls emit(key, value) for every item, in the order the entries of a key shall have.
// csr_count: ptr[key + 1] - ptr[key] = items of that key.  csr_fill: put(place, value) for every item.
template <typename I, typename Each> void csr_count(size_t n_keys, std::vector<I>& ptr, Each each)
{
    ptr.assign(n_keys + 1, 0);
    each([&](int64_t key, int64_t) { ++ptr[(size_t)key + 1]; });
    for (size_t k = 0; k < n_keys; ++k) ptr[k + 1] += ptr[k];
}
template <typename I, typename Each, typename Put> void csr_fill(const std::vector<I>& ptr, Each each, Put put)
{
    std::vector<I> fill(ptr.begin(), ptr.end() - 1);
    each([&](int64_t key, int64_t value) { put((int64_t)fill[(size_t)key]++, value); });
}

// ---- internal frame order (srk_frame_reorder above; one rank only: shards would each find another order): the cameras in
// that order and, when it is not the caller's, every landmark's observations re-sorted by internal frame (of_fr, ouv_fr)
void plan_frame_order(const SrkSceneIn& in, const SrkPlanOptions& opt, Plan& p, std::vector<int32_t>& of_fr, std::vector<double>& ouv_fr)
{
    const int32_t M = in.M;
    const int64_t N = in.N, O = in.row_ptr[N];
    std::vector<int32_t> to_int;
    bool renumber = false;
    if (opt.frame_order && !opt.frame_order->empty()) {
        to_int = *opt.frame_order;
        for (int32_t j = 0; j < M; ++j) renumber = renumber || to_int[(size_t)j] != j;
        p.frame_order_supplied = renumber;
    } else if (!opt.multi_rank)
        renumber = srk_frame_reorder(opt.frame_order_mode, N, M, in.row_ptr, in.obs_frame, to_int, opt.rel_a, opt.rel_b, opt.n_rel);
    if (renumber) {
        p.frame_int = to_int;
        p.frame_user.assign((size_t)M, 0);
        for (int32_t j = 0; j < M; ++j) p.frame_user[(size_t)to_int[(size_t)j]] = j;
        p.g0 = to_int[0];
        p.g1 = to_int[1];
    }
    p.camR.resize(9 * (size_t)M);
    p.camT.resize(3 * (size_t)M);
    p.K.resize(9 * (size_t)M);
    for (int32_t j = 0; j < M; ++j) {
        const int64_t u = renumber ? p.frame_user[(size_t)j] : j;
        std::memcpy(&p.camR[9 * (size_t)j], in.camR + 9 * u, 72);
        std::memcpy(&p.camT[3 * (size_t)j], in.camT + 3 * u, 24);
        std::memcpy(&p.K[9 * (size_t)j], in.K + 9 * u, 72);
    }
    if (!renumber) return;
    of_fr.resize((size_t)O);
    ouv_fr.resize((size_t)(2 * O));
    p.obs_rank.resize((size_t)O);
    std::vector<std::pair<int32_t, int64_t>> key;
    for (int64_t i = 0; i < N; ++i) {
        key.clear();
        for (int64_t o = in.row_ptr[i]; o < in.row_ptr[i + 1]; ++o) key.emplace_back(to_int[(size_t)in.obs_frame[o]], o);
        std::sort(key.begin(), key.end());
        for (size_t a = 0; a < key.size(); ++a) {
            const int64_t dst = in.row_ptr[i] + (int64_t)a, src = key[a].second;
            of_fr[(size_t)dst] = key[a].first;
            ouv_fr[(size_t)(2 * dst)] = in.obs_uv[2 * src];
            ouv_fr[(size_t)(2 * dst + 1)] = in.obs_uv[2 * src + 1];
            p.obs_rank[(size_t)src] = (int32_t)a;
        }
    }
}

// ---- internal landmark order: sorted by frame list, so that landmarks seeing exactly the same frames are
// contiguous (the grouped Schur kernel accumulates a run of them in registers and flushes once); the scene in that order
void plan_landmark_order(int64_t N, const int64_t* row_ptr, const int32_t* obs_frame, const double* obs_uv, const double* pts,
                         Plan& p, const std::function<void(const char*)>& stage)
{
    const int64_t O = row_ptr[N];
    std::vector<int64_t>& order = p.perm;
    order.resize((size_t)N);
    std::iota(order.begin(), order.end(), (int64_t)0);
    auto list_less = [&](int64_t x, int64_t y) {
        int64_t ox = row_ptr[x], oy = row_ptr[y];
        int64_t nx = row_ptr[x + 1] - ox, ny = row_ptr[y + 1] - oy;
        if (nx == 0 || ny == 0) return nx < ny;
        if (obs_frame[ox] != obs_frame[oy]) return obs_frame[ox] < obs_frame[oy];
        if (nx != ny) return nx < ny;
        for (int64_t k = 1; k < nx; ++k)
            if (obs_frame[ox + k] != obs_frame[oy + k]) return obs_frame[ox + k] < obs_frame[oy + k];
        return false;
    };
    // (large scenes: chunks sorted by a few host threads, then merged pairwise -- both stable, so the order is the one a
    // single stable_sort gives)
    const int n_thr = N >= 32768 ? (int)std::min<unsigned>(8, std::max<unsigned>(1, std::thread::hardware_concurrency())) : 1;
    if (n_thr > 1) {
        std::vector<int64_t> cut((size_t)n_thr + 1);
        for (int t = 0; t <= n_thr; ++t) cut[(size_t)t] = N * t / n_thr;
        std::vector<std::thread> th;
        for (int t = 0; t < n_thr; ++t)
            th.emplace_back([&, t] { std::stable_sort(order.begin() + cut[(size_t)t], order.begin() + cut[(size_t)t + 1], list_less); });
        for (auto& x : th) x.join();
        for (int w = 1; w < n_thr; w *= 2) {
            th.clear();
            for (int t = 0; t + w < n_thr; t += 2 * w)
                th.emplace_back([&, t, w] {
                    std::inplace_merge(order.begin() + cut[(size_t)t], order.begin() + cut[(size_t)(t + w)],
                                       order.begin() + cut[(size_t)std::min(t + 2 * w, n_thr)], list_less);
                });
            for (auto& x : th) x.join();
        }
    } else
        std::stable_sort(order.begin(), order.end(), list_less);
    if (stage) stage("sort landmarks by frame list");
    p.row_ptr_user.assign(row_ptr, row_ptr + N + 1);
    std::vector<int64_t>& rp = p.row_ptr_int;
    rp.assign((size_t)N + 1, 0);
    p.obs_frame.resize((size_t)O);
    p.obs_uv.resize((size_t)(2 * O));
    p.pts.resize((size_t)(3 * N));
    for (int64_t i = 0; i < N; ++i) {
        const int64_t u = order[(size_t)i];
        rp[(size_t)i + 1] = rp[(size_t)i] + (row_ptr[u + 1] - row_ptr[u]);
    }
    auto permute_range = [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            const int64_t u = order[(size_t)i];
            const int64_t cnt = row_ptr[u + 1] - row_ptr[u];
            std::memcpy(&p.obs_frame[(size_t)rp[(size_t)i]], obs_frame + row_ptr[u], (size_t)(4 * cnt));
            std::memcpy(&p.obs_uv[(size_t)(2 * rp[(size_t)i])], obs_uv + 2 * row_ptr[u], (size_t)(16 * cnt));
            std::memcpy(&p.pts[(size_t)(3 * i)], pts + 3 * u, 24);
        }
    };
    if (n_thr > 1) {
        std::vector<std::thread> th;
        for (int t = 0; t < n_thr; ++t) th.emplace_back(permute_range, N * t / n_thr, N * (t + 1) / n_thr);
        for (auto& x : th) x.join();
    } else
        permute_range(0, N);
    if (stage) stage("permute observations");
}

// A run = consecutive candidates (landmarks in the internal order; cand NULL = every landmark) over the UNION of their frame
// lists.  The union may hold cap frames and the run max_len landmarks; a landmark that widens the union costs every landmark
// of the run, so from free_len landmarks on the run takes one only while the union stays within free_nf frames.
struct RunRule { int64_t cap, max_len, free_len, free_nf; };
// grows the run that starts at candidate c0: returns its end (exclusive), uni = its frame set (ascending); merged is scratch
size_t grow_run(const Plan& p, const int32_t* cand, size_t n_cand, size_t c0, const RunRule& r, std::vector<int32_t>& uni,
                std::vector<int32_t>& merged)
{
    const std::vector<int64_t>& rp = p.row_ptr_int;
    const auto of = p.obs_frame.begin();
    auto landmark = [&](size_t c) { return cand ? (size_t)cand[c] : c; };
    uni.assign(of + rp[landmark(c0)], of + rp[landmark(c0) + 1]);
    size_t c = c0 + 1;
    while (c < n_cand && (int64_t)(c - c0) < r.max_len) {
        const size_t j = landmark(c);
        const int64_t nfj = rp[j + 1] - rp[j];
        if (nfj == 0 || nfj > r.cap) break;
        // (the common case first: the same frame list as the run so far -- nothing to merge)
        if (nfj == (int64_t)uni.size() && std::equal(uni.begin(), uni.end(), of + rp[j])) { ++c; continue; }
        merged.clear();
        std::set_union(uni.begin(), uni.end(), of + rp[j], of + rp[j + 1], std::back_inserter(merged));
        if ((int64_t)merged.size() > r.cap) break;
        if (merged.size() > uni.size() && (int64_t)(c - c0) >= r.free_len && (int64_t)merged.size() > r.free_nf) break;
        uni.swap(merged);
        ++c;
    }
    return c;
}

// landmarks [i, j) of a run over the frame set uni: mask_of[landmark] = the slots of uni it sees, slot_of[observation] (may be
// NULL) = the slot of its frame.  Returns whether every landmark sees all of uni (a "uniform" run: union == list).
bool fill_slots(const Plan& p, int64_t i, int64_t j, const std::vector<int32_t>& uni, uint32_t* mask_of, uint8_t* slot_of)
{
    const std::vector<int64_t>& rp = p.row_ptr_int;
    bool uniform = true;
    for (int64_t q = i; q < j; ++q) {
        uint32_t mask = 0;
        if (rp[(size_t)q + 1] - rp[(size_t)q] == (int64_t)uni.size()) { // as many frames as the union: the union itself
            for (int64_t o = rp[(size_t)q], k = 0; slot_of && o < rp[(size_t)q + 1]; ++o, ++k) slot_of[o] = (uint8_t)k;
            mask = (uint32_t)((1ull << uni.size()) - 1);
        } else {
            for (int64_t o = rp[(size_t)q]; o < rp[(size_t)q + 1]; ++o) {
                const int slot = (int)(std::lower_bound(uni.begin(), uni.end(), p.obs_frame[(size_t)o]) - uni.begin());
                if (slot_of) slot_of[o] = (uint8_t)slot;
                mask |= 1u << slot;
            }
            uniform = false;
        }
        mask_of[q] = mask;
    }
    return uniform;
}
// one more row of a run table: frames[run][stride] = the frame set, -1 behind it; nf negative = ragged run
void push_run(std::vector<int32_t>& first, std::vector<int32_t>& count, std::vector<int32_t>& nf, std::vector<int32_t>& frames,
              int stride, int64_t i, int64_t j, bool uniform, const std::vector<int32_t>& uni)
{
    first.push_back((int32_t)i);
    count.push_back((int32_t)(j - i));
    nf.push_back(uniform ? (int32_t)uni.size() : -(int32_t)uni.size());
    for (int k = 0; k < stride; ++k) frames.push_back(k < (int)uni.size() ? uni[(size_t)k] : -1);
}

// Runs of consecutive landmarks (internal order) whose frame lists fit a common set of <= SRK_GRP_MAXNF_HOST
// frames -> grouped Schur kernel: the run's blocks are accumulated over that UNION of frames, a landmark that does
// not see one of them contributes zeros there.  Identical lists (the circle-grid scenes) are the special case
// union == list ("uniform" run: no slot table needed); ragged feature tracks, where hardly two landmarks see
// exactly the same frames, still share a window of frames.  Landmarks with more frames -> long_cand.
void plan_schur_runs(Plan& p)
{
    const std::vector<int64_t>& rp = p.row_ptr_int;
    const int64_t N = (int64_t)rp.size() - 1;
    p.obs_slot.assign(p.obs_frame.size(), 0);
    p.pt_mask.assign((size_t)N, 0);
    std::vector<int32_t> uni, merged;
    for (int64_t i = 0; i < N;) {
        const int64_t nfi = rp[(size_t)i + 1] - rp[(size_t)i];
        if (nfi == 0) { ++i; continue; }
        if (nfi > SRK_GRP_MAXNF_HOST) { p.long_cand.push_back((int32_t)i); ++i; continue; }
        const int64_t cap = nfi > SRK_GRP_NF1_HOST ? SRK_GRP_MAXNF_HOST : SRK_GRP_NF1_HOST;
        // a wider frame set costs every landmark of the run more flops; it only pays while the run is still
        // small against its one-off flush (~ the work of a dozen landmarks)
        const int64_t j = (int64_t)grow_run(p, nullptr, (size_t)N, (size_t)i, { cap, SRK_GRP_MAXPTS_HOST, 24, 0 }, uni, merged);
        const bool uniform = fill_slots(p, i, j, uni, p.pt_mask.data(), p.obs_slot.data());
        push_run(p.grp_first, p.grp_count, p.grp_nf, p.grp_frames, SRK_GRP_MAXNF_HOST, i, j, uniform, uni);
        if ((int64_t)uni.size() > SRK_GRP_NF1_HOST) ++p.n_groups_wide;
        else if ((int64_t)uni.size() > SRK_WS_NF_HOST) ++p.n_groups_mid;
        i = j;
    }
}

// A small scene (the dino set: 36 frames, 4983 points; the point sets of the multi-view-factorisation calls) has a few
// dozen full-length runs: a few dozen workgroups on 256 CUs, each staging up to 128 landmarks four at a time -- the sum
// takes as long as one workgroup's 32 rounds (config 1: 114 us for 16 k observations).  Such runs are cut into `split`
// equal parts over the SAME frame set (slots and masks stay as they are; a cut that left a remainder to merge with the
// next frame list made ragged and wider runs: measured, worse).  What stops the cut: every part flushes the whole tile
// triangle of its frame set, and the parts of one round of workgroups flush together -- the fp64 atomics of a burst
// drain at ~0.5 TB/s (100 frames x 5000 points, 20-frame tracks: 74 / 72 / 78 / 96 / 155 us with 1 / 2 / 3 / 4 / 8
// parts; config 1, 4-frame tracks: 114 / 68 / 57 / 49 us with 1 / 2 / 3 / 4 parts, `tools/run_len_probe.py`) -- and a
// second round of workgroups.  The model below is that shape: a double round of eight landmarks ~5.5 us, 2 KB a tile.
void split_schur_runs(Plan& p, const SrkPlanOptions& opt)
{
    const int cus = opt.cus;
    auto cost = [&](int split) {
        double worst = 0, tiles = 0;
        int64_t parts = 0;
        for (size_t r = 0; r < p.grp_first.size(); ++r) {
            const int64_t nfu = std::abs(p.grp_nf[r]), nt = (10 * nfu + 15) / 16, len = (p.grp_count[r] + split - 1) / split;
            const int64_t k = std::min<int64_t>(split, (p.grp_count[r] + len - 1) / len);
            parts += k;
            tiles += (double)(k * nt * (nt + 1) / 2);
            worst = std::max(worst, 4.5 + 5.5 * (double)((len + 7) / 8));
        }
        return worst * (double)((parts + cus - 1) / cus) + tiles * 2048.0 / 0.5e6; // us
    };
    int split = 1;
    if (!p.grp_first.empty() && (int)p.grp_first.size() < cus) {
        double best = cost(1);
        for (int sp = 2; sp <= 8; ++sp) {
            const double c = cost(sp);
            if (c < 0.9 * best) best = c, split = sp;
        }
    }
    if (opt.run_split > 0) split = opt.run_split; // development: fixed cut
    if (split <= 1) return;
    std::vector<int32_t> f2, c2, n2, fr2;
    for (size_t r = 0; r < p.grp_first.size(); ++r) {
        const int64_t len = (p.grp_count[r] + split - 1) / split;
        for (int64_t a = 0; a < p.grp_count[r]; a += len) {
            f2.push_back(p.grp_first[r] + (int32_t)a);
            c2.push_back((int32_t)std::min<int64_t>(len, p.grp_count[r] - a));
            n2.push_back(p.grp_nf[r]);
            fr2.insert(fr2.end(), p.grp_frames.begin() + (ptrdiff_t)(r * SRK_GRP_MAXNF_HOST), p.grp_frames.begin() + (ptrdiff_t)((r + 1) * SRK_GRP_MAXNF_HOST));
            if (a > 0) {
                if (std::abs(p.grp_nf[r]) > SRK_GRP_NF1_HOST) ++p.n_groups_wide;
                else if (std::abs(p.grp_nf[r]) > SRK_WS_NF_HOST) ++p.n_groups_mid;
            }
        }
    }
    p.grp_first.swap(f2); p.grp_count.swap(c2); p.grp_nf.swap(n2); p.grp_frames.swap(fr2);
}

// Long tracks (> SRK_GRP_MAXNF_HOST frames; every track of the demos' all-visible scenes): runs of consecutive
// candidates over the union of their frame lists (<= SRK_LONG_MAXNF_HOST frames), cut into blocks of 8 frames; one
// work item per pair of blocks (k_schur_long).  A track over more frames than a run holds keeps the per-landmark kernel.
void plan_long_runs(Plan& p, const SrkPlanOptions& opt)
{
    const std::vector<int64_t>& rp = p.row_ptr_int;
    std::vector<int32_t>& long_cand = p.long_cand;
    if (opt.no_long) { // development: everything through the per-landmark kernel
        p.gen_list.insert(p.gen_list.end(), long_cand.begin(), long_cand.end());
        long_cand.clear();
    }
    std::vector<int32_t> uni, merged;
    for (size_t ci = 0; ci < long_cand.size();) {
        const int64_t i = long_cand[ci];
        const int64_t nfi = rp[(size_t)i + 1] - rp[(size_t)i];
        if (nfi > SRK_LONG_MAXNF_HOST) { p.gen_list.push_back((int32_t)i); ++ci; continue; }
        // every landmark of the run pays for the whole union: let it grow freely only while the run is small
        const size_t cj = grow_run(p, long_cand.data(), long_cand.size(), ci,
                                   { SRK_LONG_MAXNF_HOST, SRK_LONG_PTS_HOST, 16, nfi + nfi / 4 + SRK_LONG_FB_HOST }, uni, merged);
        const int nfu = (int)uni.size();
        p.lg_np.push_back((int32_t)(cj - ci));
        p.lg_nf.push_back((int32_t)nfu);
        for (int k = 0; k < SRK_LONG_PTS_HOST; ++k) p.lg_pts.push_back(ci + k < cj ? long_cand[ci + (size_t)k] : 0);
        for (int k = 0; k < SRK_LONG_MAXNF_HOST; ++k) p.lg_frames.push_back(k < nfu ? uni[(size_t)k] : -1);
        ci = cj;
    }
}
// Frame blocks of 8 or of 16 frames (round 4).  A workgroup stages both blocks of its pair for every landmark of the run:
// with 8-frame blocks that is two staged blocks for 25 MFMA tiles and the kernel spent its time staging (SQ counters on
// 200 frames x 20 000 points, every point in every frame: 7 vector-ALU, 0.85 memory and 0.9 LDS instructions per MFMA,
// matrix pipes 33 % busy); a pair of 16-frame blocks is two staged blocks for 100 tiles.  The larger blocks need enough
// pairs to fill the chip: small scenes (the 36- and 60-frame demo scenes) keep the 8-frame blocks.
void plan_long_items(Plan& p)
{
    const std::vector<int64_t>& rp = p.row_ptr_int;
    int64_t items16 = 0, nf_sum = 0;
    for (size_t r = 0; r < p.lg_np.size(); ++r) {
        const int64_t nb16 = (p.lg_nf[r] + 15) / 16;
        items16 += nb16 * (nb16 + 1) / 2;
        nf_sum += p.lg_nf[r];
    }
    // (and frame sets long enough that the padding to 16 and the coarser diagonal pairs do not eat the gain.  Counting a
    // staged block-frame as ~3 MFMA tiles -- what the counters above say -- 40 frames cost the same either way, 64 frames
    // 30 % less with the larger blocks)
    p.long_fb = (items16 >= 1024 && nf_sum >= 56 * (int64_t)p.lg_np.size()) ? 16 : SRK_LONG_FB_HOST;
    const int FBh = p.long_fb;
    for (size_t r = 0; r < p.lg_np.size(); ++r) {
        const int32_t run = (int32_t)r;
        const int nfu = p.lg_nf[r], nb = (nfu + FBh - 1) / FBh, nfp = nb * FBh;
        const int32_t* uni_b = p.lg_frames.data() + r * SRK_LONG_MAXNF_HOST;
        p.lg_obs_off.push_back((int64_t)p.lg_obs.size());
        for (int k = 0; k < p.lg_np[r]; ++k) {
            const int64_t q = p.lg_pts[r * SRK_LONG_PTS_HOST + (size_t)k];
            const size_t base = p.lg_obs.size();
            p.lg_obs.resize(base + (size_t)nfp, -1);
            for (int64_t o = rp[(size_t)q]; o < rp[(size_t)q + 1]; ++o) {
                const int slot = (int)(std::lower_bound(uni_b, uni_b + nfu, p.obs_frame[(size_t)o]) - uni_b);
                p.lg_obs[base + (size_t)slot] = (int32_t)o;
            }
        }
        for (int a = 0; a < nb; ++a)
            for (int b = 0; b <= a; ++b) {
                p.lg_item.push_back(run); p.lg_item.push_back(a); p.lg_item.push_back(b); p.lg_item.push_back(0);
            }
    }
}

// observation side tables (obs -> point, observations per frame) and the frame range of every SRK_JF_OBS_HOST-observation
// workgroup of the fused Jacobian kernel
void plan_side_tables(Plan& p, int32_t M)
{
    const std::vector<int64_t>& rp = p.row_ptr_int;
    const int64_t N = (int64_t)rp.size() - 1, O = rp[(size_t)N];
    p.obs_pt.resize((size_t)O);
    csr_count((size_t)M, p.col_ptr, [&](auto emit) {
        for (int64_t i = 0; i < N; ++i)
            for (int64_t o = rp[(size_t)i]; o < rp[(size_t)i + 1]; ++o) {
                p.obs_pt[(size_t)o] = (int32_t)i;
                emit(p.obs_frame[(size_t)o], o);
            }
    });
    p.max_frame_obs = 0;
    for (int32_t j = 0; j < M; ++j) p.max_frame_obs = std::max(p.max_frame_obs, p.col_ptr[(size_t)j + 1] - p.col_ptr[(size_t)j]);
    p.jac_fused = true;
    const int32_t* of = p.obs_frame.data();
    for (int64_t o0 = 0; o0 < O; o0 += SRK_JF_OBS_HOST) {
        const int64_t o1 = std::min<int64_t>(O, o0 + SRK_JF_OBS_HOST);
        int32_t lo = of[o0], hi = of[o0];
        for (int64_t o = o0; o < o1; ++o) {
            lo = std::min(lo, of[o]);
            hi = std::max(hi, of[o]);
        }
        if (hi - lo >= SRK_JF_SLOTS_HOST) p.jac_fused = false;
        if (p.obs_pt[(size_t)o1 - 1] - p.obs_pt[(size_t)o0] + 1 > SRK_JF_PMAX_HOST) p.jac_fused = false;
        p.wg_jmin.push_back(lo);
    }
}

// cuts len landmarks from `first` on, all over nf frames, into tasks of the run-based derivative kernel: equal pieces of a
// multiple of the 64 / nf landmarks a step takes, about `target` landmarks each.  group >= 0: the run they are pieces of.
void cut_pieces(Plan& p, int64_t first, int64_t len, int64_t nf, int64_t target, int32_t group)
{
    const int64_t g = 64 / nf;
    const int64_t most = SRK_JR_TASK_PTS_MAX_HOST / g * g; // the kernel stages a task's landmarks in LDS
    const int64_t pieces = std::max<int64_t>((len + most - 1) / most, (len + target / 2) / target);
    const int64_t piece = std::max<int64_t>(g, ((len + pieces - 1) / pieces + g - 1) / g * g);
    for (int64_t a = 0; a < len; a += piece) {
        p.jr_first.push_back((int32_t)(first + a));
        p.jr_count.push_back((int32_t)std::min<int64_t>(piece, len - a));
        if (group >= 0) p.jr_group.push_back(group);
    }
}
// jr_jmin = the first frame of every four consecutive tasks (one workgroup), span(task, lo, hi) being a task's frame range;
// false, and no further, when a workgroup would touch SRK_JF_SLOTS_HOST consecutive frames or more
template <typename Span> bool task_windows(Plan& p, int32_t M, Span span)
{
    for (size_t t0 = 0; t0 < p.jr_first.size(); t0 += 4) {
        int32_t lo = M, hi = -1;
        for (size_t t = t0; t < std::min(p.jr_first.size(), t0 + 4); ++t) {
            int32_t a, b;
            span(t, a, b);
            lo = std::min(lo, a);
            hi = std::max(hi, b);
        }
        p.jr_jmin.push_back(lo);
        if (hi - lo >= SRK_JF_SLOTS_HOST) return false;
    }
    return true;
}

// tasks of the run-based Jacobian kernel: maximal runs of consecutive landmarks (internal order) with identical
// frame lists, cut into pieces (a multiple of the landmarks per step).  The kernel holds two 4-wave workgroups per
// CU (a wave keeps 61 frame sums and a step of look-ahead in ~250 registers); with about one task per wave slot
// every task runs at the same time and the stores of all of them share HBM from start to end (with 1.4 rounds of
// shorter tasks the second round ran at 2 TB/s).
void plan_uniform_tasks(Plan& p, const SrkPlanOptions& opt, int32_t M, int64_t target)
{
    const std::vector<int64_t>& rp = p.row_ptr_int;
    const std::vector<int32_t>& of = p.obs_frame;
    const int64_t N = (int64_t)rp.size() - 1, O = rp[(size_t)N];
    // (the kernel addresses W with 32-bit byte offsets inside a plane and inside each half of the 30 planes)
    p.jac_runs = opt.jac_mode != 0 && O < (int64_t)1 << 27;
    p.jr_min_nf = 64;
    for (int64_t i = 0; i < N && p.jac_runs;) {
        const int64_t nf = rp[(size_t)i + 1] - rp[(size_t)i];
        if (nf == 0) { ++i; continue; }
        if (nf > 64) { p.jac_runs = false; break; }
        p.jr_min_nf = std::min<int32_t>(p.jr_min_nf, (int32_t)nf);
        int64_t j = i + 1;
        while (j < N && rp[(size_t)j + 1] - rp[(size_t)j] == nf &&
               std::equal(of.begin() + rp[(size_t)i], of.begin() + rp[(size_t)i + 1], of.begin() + rp[(size_t)j])) ++j;
        cut_pieces(p, i, j - i, nf, target, -1);
        i = j;
    }
    if (!p.jac_runs) return;
    // long enough to pay: a task flushes 65 sums per lane, which an iteration of the per-observation kernel costs.
    // (Round 3, tools/jac_modes.py: at 240 observations a task -- C2 -- the run kernel takes 45 us where the fused
    // per-observation kernel takes 64; tasks of one or two ragged landmarks, ~20 observations, 118 against 69.)
    if (p.jr_first.empty() || (opt.jac_mode != 1 && O / (int64_t)p.jr_first.size() < 128)) p.jac_runs = false;
    else
        p.jac_runs = task_windows(p, M, [&](size_t t, int32_t& lo, int32_t& hi) {
            lo = of[(size_t)rp[(size_t)p.jr_first[t]]];
            hi = of[(size_t)rp[(size_t)p.jr_first[t] + 1] - 1];
        });
}

// The derivative kernel's own runs over unions of <= SRK_JD_MAXNF_HOST frames (a lane's observation is found from a 32-bit
// mask), for scenes with tracks over more than SRK_GRP_MAXNF_HOST frames when no track is longer than that.
void plan_own_runs(Plan& p)
{
    const std::vector<int64_t>& rp = p.row_ptr_int;
    const int64_t N = (int64_t)rp.size() - 1;
    for (int32_t q : p.long_cand)
        if (rp[(size_t)q + 1] - rp[(size_t)q] > SRK_JD_MAXNF_HOST) return;
    p.jd_mask.assign((size_t)N, 0);
    std::vector<int32_t> uni, merged;
    for (int64_t i = 0; i < N;) {
        if (rp[(size_t)i + 1] == rp[(size_t)i]) { ++i; continue; }
        // (a wider set costs every landmark of the run lanes)
        const int64_t j = (int64_t)grow_run(p, nullptr, (size_t)N, (size_t)i, { SRK_JD_MAXNF_HOST, SRK_GRP_MAXPTS_HOST, 24, 0 }, uni, merged);
        const bool uniform = fill_slots(p, i, j, uni, p.jd_mask.data(), nullptr);
        push_run(p.jd_first, p.jd_count, p.jd_nf, p.jd_frames, SRK_JD_MAXNF_HOST, i, j, uniform, uni);
        i = j;
    }
    p.jr_own_runs = true;
}

// Ragged tracks: hardly two landmarks see exactly the same frames, so the uniform runs are too short to pay -- but the
// Schur kernel's runs (consecutive landmarks over the UNION of their frame lists, <= 24 frames, masks) are not.  The same
// kernel with a lane per (landmark, frame slot) CELL: tasks = pieces of those runs.  Needs every landmark in a run: the Schur
// kernels' (every landmark is in one when no track is longer than SRK_GRP_MAXNF_HOST frames), else the kernel's own.
void plan_union_tasks(Plan& p, const SrkPlanOptions& opt, int32_t M, int64_t target)
{
    const int64_t O = (int64_t)p.obs_frame.size();
    if (!((!p.jac_runs || opt.jac_mode == 2) && opt.jac_mode != 0 && O < (int64_t)1 << 27 && p.gen_list.empty())) return;
    if (!p.long_cand.empty()) plan_own_runs(p);
    const std::vector<int32_t>& rn_first = p.jr_own_runs ? p.jd_first : p.grp_first;
    const std::vector<int32_t>& rn_count = p.jr_own_runs ? p.jd_count : p.grp_count;
    const std::vector<int32_t>& rn_nf = p.jr_own_runs ? p.jd_nf : p.grp_nf;
    const std::vector<int32_t>& rn_frames = p.jr_own_runs ? p.jd_frames : p.grp_frames;
    const size_t rn_stride = p.jr_own_runs ? (size_t)SRK_JD_MAXNF_HOST : (size_t)SRK_GRP_MAXNF_HOST;
    if (!(p.jr_own_runs || p.long_cand.empty()) || rn_first.empty()) return;
    const bool uniform_ok = p.jac_runs; // (mode 2: the union tasks are preferred, the uniform ones stay as the fallback)
    std::vector<int32_t> u_first, u_count, u_jmin;
    u_first.swap(p.jr_first); u_count.swap(p.jr_count); u_jmin.swap(p.jr_jmin);
    for (size_t gi = 0; gi < rn_first.size(); ++gi) cut_pieces(p, rn_first[gi], rn_count[gi], std::abs(rn_nf[gi]), target, (int32_t)gi);
    const bool ok = (opt.jac_mode >= 1 || O / (int64_t)p.jr_first.size() >= 32) && // (the dino stand-in: 40 a task, 31 against 60 us)
                    task_windows(p, M, [&](size_t t, int32_t& lo, int32_t& hi) {
                        const size_t gi = (size_t)p.jr_group[t];
                        lo = rn_frames[gi * rn_stride];
                        hi = rn_frames[gi * rn_stride + (size_t)std::abs(rn_nf[gi]) - 1];
                    });
    p.jac_runs_masked = ok;
    if (!ok) { // back to the uniform tasks (if they were usable)
        p.jr_first.swap(u_first); p.jr_count.swap(u_count); p.jr_jmin.swap(u_jmin);
        p.jr_group.clear();
        p.jac_runs = uniform_ok;
        p.jr_own_runs = false;
    } else
        p.jac_runs = true;
}

// ---- deterministic mode: tables of the ordered second passes.  Covered: scenes whose landmarks all take the run-based
// derivative kernel and the MFMA Schur kernel (tracks over at most SRK_WS_NF_HOST frames, fp64 run sums).
void plan_det_tables(Plan& p, const SrkPlanOptions& opt, int32_t M)
{
    if (!(opt.deterministic && p.jac_runs && p.n_groups_wide == 0 && p.n_groups_mid == 0 && p.lg_item.empty() && p.gen_list.empty() &&
          !opt.schur_fp32 && !p.grp_first.empty() && p.grp_first.size() < ((size_t)1 << 20) && p.jr_first.size() < ((size_t)1 << 25)))
        return;
    for (int32_t v : p.grp_nf)
        if (std::abs(v) > SRK_WS_NF_HOST) return;
    const std::vector<int64_t>& rp = p.row_ptr_int;
    // derivative tasks by frame
    auto each_task_frame = [&](auto emit) {
        for (size_t t = 0; t < p.jr_first.size(); ++t) {
            const size_t gi = p.jr_group.empty() ? 0 : (size_t)p.jr_group[t], q = (size_t)p.jr_first[t];
            const int32_t* fr = p.jr_group.empty() ? p.obs_frame.data() + rp[q] : p.grp_frames.data() + gi * SRK_GRP_MAXNF_HOST;
            const int nf = p.jr_group.empty() ? (int)(rp[q + 1] - rp[q]) : std::abs(p.grp_nf[gi]);
            for (int f = 0; f < nf; ++f) emit(fr[f], (int64_t)(t * 64 + (size_t)f));
        }
    };
    csr_count((size_t)M, p.dj_ptr, each_task_frame);
    p.dj_ent.resize((size_t)p.dj_ptr[(size_t)M]);
    csr_fill(p.dj_ptr, each_task_frame, [&](int64_t at, int64_t v) { p.dj_ent[(size_t)at] = (int32_t)v; });
    // Schur runs by frame and by block (fa >= fb)
    auto each_run_frame = [&](auto emit) {
        for (size_t gi = 0; gi < p.grp_first.size(); ++gi)
            for (int sa = 0; sa < std::abs(p.grp_nf[gi]); ++sa) emit(p.grp_frames[gi * SRK_GRP_MAXNF_HOST + (size_t)sa], (int64_t)((uint32_t)gi | (uint32_t)sa << 20));
    };
    csr_count((size_t)M, p.ds_f_ptr, each_run_frame);
    p.ds_f_ent.resize((size_t)p.ds_f_ptr[(size_t)M]);
    csr_fill(p.ds_f_ptr, each_run_frame, [&](int64_t at, int64_t v) { p.ds_f_ent[(size_t)at] = (int32_t)v; });
    std::vector<std::pair<int64_t, int32_t>> ents;
    for (size_t gi = 0; gi < p.grp_first.size(); ++gi) {
        const int32_t* fr = p.grp_frames.data() + gi * SRK_GRP_MAXNF_HOST;
        for (int sa = 0; sa < std::abs(p.grp_nf[gi]); ++sa)
            for (int sb = 0; sb <= sa; ++sb)
                ents.emplace_back((int64_t)fr[sa] * M + fr[sb], (int32_t)((uint32_t)gi | (uint32_t)sa << 20 | (uint32_t)sb << 25));
    }
    std::stable_sort(ents.begin(), ents.end(), [](const std::pair<int64_t, int32_t>& x, const std::pair<int64_t, int32_t>& y) { return x.first < y.first; });
    p.ds_pair_ent.reserve(ents.size());
    for (size_t e = 0; e < ents.size(); ++e) {
        if (e == 0 || ents[e].first != ents[e - 1].first) {
            p.ds_pair_ptr.push_back((int32_t)e);
            p.ds_pair_fa.push_back((int32_t)(ents[e].first / M));
            p.ds_pair_fb.push_back((int32_t)(ents[e].first % M));
        }
        p.ds_pair_ent.push_back(ents[e].second);
    }
    p.ds_pair_ptr.push_back((int32_t)ents.size());
    p.ds_n_pairs = (int32_t)p.ds_pair_fa.size();
    p.det_active = true;
}

// the frame-major copy of the observations (ordered by frame, then landmark): only the two-kernel derivative path reads it
void plan_frame_major(Plan& p)
{
    if (p.jac_runs || p.jac_fused) return;
    const size_t O = p.obs_frame.size();
    p.fobs_pt.resize(O);
    p.fobs_uv.resize(2 * O);
    p.fobs_of.resize(O);
    csr_fill(p.col_ptr, [&](auto emit) { for (size_t o = 0; o < O; ++o) emit(p.obs_frame[o], (int64_t)o); },
             [&](int64_t k, int64_t o) {
                 p.fobs_of[(size_t)o] = k;
                 p.fobs_pt[(size_t)k] = p.obs_pt[(size_t)o];
                 p.fobs_uv[(size_t)(2 * k)] = p.obs_uv[(size_t)(2 * o)];
                 p.fobs_uv[(size_t)(2 * k + 1)] = p.obs_uv[(size_t)(2 * o + 1)];
             });
}

// fixed intrinsics: k_schur_mm sums the runs of at most SRK_WS_NF_HOST frames on 6-wide blocks; every other landmark (wider
// runs, long tracks, the generic list) takes the per-landmark kernel
void plan_cal_list(Plan& p)
{
    const std::vector<int64_t>& rp = p.row_ptr_int;
    const int64_t N = (int64_t)rp.size() - 1;
    std::vector<char> in_mm((size_t)N, 0);
    for (size_t r = 0; r < p.grp_first.size(); ++r)
        if (std::abs(p.grp_nf[r]) <= SRK_WS_NF_HOST)
            for (int32_t k = 0; k < p.grp_count[r]; ++k) in_mm[(size_t)(p.grp_first[r] + k)] = 1;
    for (int64_t i = 0; i < N; ++i)
        if (!in_mm[(size_t)i] && rp[(size_t)i + 1] > rp[(size_t)i]) p.cal_list.push_back((int32_t)i);
}

// covisibility of THIS shard; with several ranks the caller must supply the global one (srk_ba_set_covisibility) -- until
// then the skyline is the full lower triangle
// A relative-pose factor between frames a and b puts a block at (max, min) of the system like a shared landmark does.
void plan_min_cv(Plan& p, int32_t M, bool multi_rank, const SrkPlanOptions& opt)
{
    const std::vector<int64_t>& rp = p.row_ptr_int;
    p.min_cv.assign((size_t)M, 0);
    if (multi_rank) return;
    for (int32_t j = 0; j < M; ++j) p.min_cv[(size_t)j] = j;
    int32_t* cv = p.min_cv.data();
    const int32_t* of = p.obs_frame.data();
    for (size_t i = 0; i + 1 < rp.size(); ++i) {
        if (rp[i + 1] == rp[i]) continue;
        const int32_t first = of[rp[i]];
        for (int64_t o = rp[i]; o < rp[i + 1]; ++o) cv[of[o]] = std::min(cv[of[o]], first);
    }
    for (int64_t k = 0; k < opt.n_rel; ++k) {
        const int32_t a = p.frame_int.empty() ? opt.rel_a[k] : p.frame_int[(size_t)opt.rel_a[k]];
        const int32_t b = p.frame_int.empty() ? opt.rel_b[k] : p.frame_int[(size_t)opt.rel_b[k]];
        cv[std::max(a, b)] = std::min(cv[std::max(a, b)], std::min(a, b));
    }
}

} // namespace

void srk_plan_scene(const SrkSceneIn& in, const SrkPlanOptions& opt, SrkScenePlan& p, const std::function<void(const char*)>& stage)
{
    const int32_t M = in.M;
    {
        std::vector<int32_t> of_fr;
        std::vector<double> ouv_fr;
        plan_frame_order(in, opt, p, of_fr, ouv_fr);
        if (stage) stage("normalise, frame order");
        plan_landmark_order(in.N, in.row_ptr, of_fr.empty() ? in.obs_frame : of_fr.data(), ouv_fr.empty() ? in.obs_uv : ouv_fr.data(),
                            in.pts, p, stage);
    }
    plan_schur_runs(p);
    split_schur_runs(p, opt);
    plan_long_runs(p, opt);
    plan_long_items(p);
    p.n_long_runs = (int64_t)p.lg_np.size();
    p.n_long_items = (int64_t)p.lg_item.size() / 4;
    p.n_groups = (int64_t)p.grp_first.size();
    for (int32_t v : p.grp_nf) {
        if (v > 0 && v <= SRK_WS_NF_HOST) ++p.n_mm_uniform;
        if (v < 0 && -v <= SRK_WS_NF_HOST) ++p.n_mm_ragged;
    }
    p.n_generic = (int64_t)p.gen_list.size();
    if (stage) stage("Schur runs");
    plan_side_tables(p, M);
    if (stage) stage("side tables, frame windows");
    int64_t with_obs = 0;
    for (int64_t i = 0; i < in.N; ++i) with_obs += p.row_ptr_int[(size_t)i + 1] > p.row_ptr_int[(size_t)i];
    const int64_t slots = 8 * (int64_t)opt.cus; // waves resident at once
    const int64_t target = std::min<int64_t>(SRK_JR_TASK_PTS_MAX_HOST, std::max<int64_t>(SRK_JR_TASK_PTS_MIN_HOST, (with_obs + slots - 1) / slots));
    plan_uniform_tasks(p, opt, M, target);
    plan_union_tasks(p, opt, M, target);
    p.jr_tasks = p.jac_runs ? (int32_t)p.jr_first.size() : 0;
    plan_det_tables(p, opt, M);
    if (stage) stage("deterministic-mode tables");
    plan_frame_major(p);
    if (opt.fixed_k) plan_cal_list(p);
    p.n_cal_list = (int64_t)p.cal_list.size();
    plan_min_cv(p, M, opt.multi_rank, opt);
    if (stage) stage("derivative tasks");
}
