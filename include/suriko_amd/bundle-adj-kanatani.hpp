// bundle-adj-kanatani.hpp -- C++17 adapter with the class API of whigg/surikatoko's BundleAdjustmentKanatani
// (cpp_impl/suriko-engine/include/suriko/bundle-adj-kanatani.h:96-261) on top of the C ABI of libsrk_ba.so
// (include/srk_ba.h).  Header-only; no Eigen, glog or GSL (not available in this image): the containers below
// carry exactly the data the reference's FragmentMap / CornerTrackRepository / SE3Transform hand to the BA call.
//
// A maintainer of the reference swaps the body of suriko::BundleAdjustmentKanatani::ComputeInplace for a call to
// suriko_amd::BundleAdjustmentKanatani::ComputeInplace after copying its Eigen containers into these plain ones
// (INTEGRATION.md shows the ~40-line shim).  Semantics kept: in-place update of points and inverse camera poses,
// exactly one of shared_K / Ks, `bool` result + OptimizationStatusString(), K never modified (reference quirk,
// bundle-adj-kanatani.cpp:2027-2034), pnt_ind = order of tracks that have a SalientPointId (:1161-1169) while
// coordinates are fetched by salient-point id (:1171).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../srk_ba.h"

namespace suriko_amd {

using Scalar = double; // rt-config.h:41-48 (default)

struct Point3 { Scalar x = 0, y = 0, z = 0; };
struct Point2f { Scalar x = 0, y = 0; };
using Matrix3 = std::array<Scalar, 9>; // row-major

/// obs-geom.h:177-190.  Inverse orientation: world -> camera.
struct SE3Transform {
    Point3 T;
    Matrix3 R{ 1, 0, 0, 0, 1, 0, 0, 0, 1 };
};

/// obs-geom.h:207-243: id -> index = id - offset - 1 (obs-geom.cpp:247-251), default offset 1'000'000.
class FragmentMap {
public:
    explicit FragmentMap(size_t fragment_id_offset = 1000000) : offset_(fragment_id_offset) {}
    size_t AddSalientPoint(const Point3& p) { pts_.push_back(p); return pts_.size() + offset_; }
    size_t SalientPointsCount() const { return pts_.size(); }
    Point3& GetSalientPoint(size_t id) { return pts_.at(id - offset_ - 1); }
    const Point3& GetSalientPoint(size_t id) const { return pts_.at(id - offset_ - 1); }
    /// the place of a salient point in the map (the order of AddSalientPoint): what per-point arrays are indexed by
    size_t SalientPointIndex(size_t id) const { return id - offset_ - 1; }
private:
    std::vector<Point3> pts_;
    size_t offset_;
};

/// obs-geom.h:251-283: a start frame + one optional corner per following frame (gaps allowed).
struct CornerTrack {
    size_t TrackId = 0;
    std::optional<size_t> SalientPointId;
    ptrdiff_t StartFrameInd = -1;
    std::vector<std::optional<Point2f>> CoordPerFramePixels;
    void AddCorner(size_t frame_ind, const Point2f& v) {
        if (StartFrameInd == -1) StartFrameInd = (ptrdiff_t)frame_ind;
        if ((ptrdiff_t)frame_ind < StartFrameInd) throw std::invalid_argument("corner before the start frame");
        CoordPerFramePixels.resize(frame_ind - (size_t)StartFrameInd + 1);
        CoordPerFramePixels.back() = v;
    }
    std::optional<Point2f> GetCorner(size_t frame_ind) const {
        ptrdiff_t k = (ptrdiff_t)frame_ind - StartFrameInd;
        if (StartFrameInd == -1 || k < 0 || (size_t)k >= CoordPerFramePixels.size()) return std::nullopt;
        return CoordPerFramePixels[(size_t)k];
    }
};
struct CornerTrackRepository {
    std::vector<CornerTrack> CornerTracks;
    CornerTrack& AddCornerTrackObj() { CornerTracks.emplace_back(); CornerTracks.back().TrackId = CornerTracks.size() - 1; return CornerTracks.back(); }
};

/// bundle-adj-kanatani.h:68-92
class BundleAdjustmentKanataniTermCriteria {
public:
    void AllowedReprojErrRelativeChange(std::optional<Scalar> v) { rel_ = v; }
    std::optional<Scalar> AllowedReprojErrRelativeChange() const { return rel_; }
    void MaxHessianFactor(std::optional<Scalar> v) { maxf_ = v; }
    std::optional<Scalar> MaxHessianFactor() const { return maxf_; }
private:
    std::optional<Scalar> rel_, maxf_;
};

class BundleAdjustmentKanatani {
public:
    explicit BundleAdjustmentKanatani(int device_id = 0) : h_(srk_ba_create(device_id)) {
        if (!h_) throw std::runtime_error("srk_ba_create failed: no usable HIP device (there is no CPU fallback)");
    }
    ~BundleAdjustmentKanatani() { srk_ba_destroy(h_); }
    BundleAdjustmentKanatani(const BundleAdjustmentKanatani&) = delete;
    BundleAdjustmentKanatani& operator=(const BundleAdjustmentKanatani&) = delete;

    /// bundle-adj-kanatani.h:179-184.  Throws std::invalid_argument where the reference CHECK-aborts
    /// (f0 ~ 0, both or neither K given, :420-421).
    bool ComputeInplace(Scalar f0, FragmentMap& map, std::vector<SE3Transform>& inverse_orient_cams,
                        const CornerTrackRepository& track_rep, const Matrix3* shared_intrinsic_cam_mat,
                        std::vector<Matrix3>* intrinsic_cam_mats, const BundleAdjustmentKanataniTermCriteria& term_crit,
                        int64_t max_iterations = 0) {
        Flat f = Flatten(f0, map, inverse_orient_cams, track_rep, shared_intrinsic_cam_mat, intrinsic_cam_mats);
        ApplyConstantBlocks(map, f, inverse_orient_cams.size());
        ApplyPositionPriors(map, f);
        ApplyRelativePoseFactors();
        ApplyJointPosePriors();
        Scalar a = term_crit.AllowedReprojErrRelativeChange().value_or(0), m = term_crit.MaxHessianFactor().value_or(0);
        int rc = srk_ba_compute_inplace(h_, f0, (int64_t)f.ids.size(), f.pts.data(), (int32_t)inverse_orient_cams.size(),
                                        f.R.data(), f.T.data(), f.K.data(), f.shared, f.row_ptr.data(), f.frames.data(),
                                        f.uv.data(), term_crit.AllowedReprojErrRelativeChange() ? &a : nullptr,
                                        term_crit.MaxHessianFactor() ? &m : nullptr, max_iterations, &report_);
        if (rc < 0) Raise(rc);
        status_ = srk_ba_status_string(report_.status);
        f0_ = f0;
        points_count_ = f.ids.size();
        frames_count_ = inverse_orient_cams.size();
        pnt_ind_of_.assign(map.SalientPointsCount(), -1); // for Covariances: salient point -> pnt_ind of the resident scene
        for (size_t i = 0; i < f.ids.size(); ++i) pnt_ind_of_[map.SalientPointIndex(f.ids[i])] = (int64_t)i;
        // write back: points by salient-point id, cameras in place (K is never modified)
        for (size_t i = 0; i < f.ids.size(); ++i) {
            Point3& p = map.GetSalientPoint(f.ids[i]);
            p.x = f.pts[3 * i]; p.y = f.pts[3 * i + 1]; p.z = f.pts[3 * i + 2];
        }
        for (size_t j = 0; j < inverse_orient_cams.size(); ++j) {
            for (int e = 0; e < 9; ++e) inverse_orient_cams[j].R[(size_t)e] = f.R[9 * j + (size_t)e];
            inverse_orient_cams[j].T = { f.T[3 * j], f.T[3 * j + 1], f.T[3 * j + 2] };
        }
        return rc == 0;
    }

    /// bundle-adj-kanatani.h:167-172 (static in the reference; needs a device here)
    Scalar ReprojError(Scalar f0, const FragmentMap& map, const std::vector<SE3Transform>& inverse_orient_cams,
                       const CornerTrackRepository& track_rep, const Matrix3* shared_intrinsic_cam_mat = nullptr,
                       const std::vector<Matrix3>* intrinsic_cam_mats = nullptr, size_t* seen_points_count = nullptr) {
        Flat f = Flatten(f0, map, inverse_orient_cams, track_rep, shared_intrinsic_cam_mat, intrinsic_cam_mats);
        int64_t seen = 0;
        Scalar e = srk_ba_reproj_error(h_, f0, (int64_t)f.ids.size(), f.pts.data(), (int32_t)inverse_orient_cams.size(),
                                       f.R.data(), f.T.data(), f.K.data(), f.shared, f.row_ptr.data(), f.frames.data(),
                                       f.uv.data(), &seen);
        if (std::isnan(e)) throw std::runtime_error(std::string("srk_ba_reproj_error: ") + srk_ba_last_error(h_));
        if (seen_points_count) *seen_points_count = (size_t)seen;
        f0_ = f0;
        return e;
    }
    /// MultiViewIterativeFactorizer::ReprojError (multi-view-factorization.cpp:415-475): the score the MVF driver takes
    /// before deciding to run BA; shared K only, observations with |z| <= 1e-5 skipped, false when nothing was summed.
    bool ReprojErrorMvf(Scalar f0, const FragmentMap& map, const std::vector<SE3Transform>& cam_orient_cfw,
                        const CornerTrackRepository& track_rep, const Matrix3* shared_intrinsic_cam_mat, Scalar* reproj_err) {
        Flat f = Flatten(f0, map, cam_orient_cfw, track_rep, shared_intrinsic_cam_mat, (const std::vector<Matrix3>*)nullptr);
        int64_t n = 0;
        int rc = srk_ba_reproj_error_mvf(h_, f0, (int64_t)f.ids.size(), f.pts.data(), (int32_t)cam_orient_cfw.size(),
                                         f.R.data(), f.T.data(), f.K.data(), f.shared, f.row_ptr.data(), f.frames.data(),
                                         f.uv.data(), 1e-5, reproj_err, &n);
        if (rc < 0) Raise(rc);
        return rc == 1;
    }
    Scalar ReprojErrorPixPerPoint(Scalar reproj_err, size_t seen) const { return f0_ * std::sqrt(reproj_err / (Scalar)seen); } // .cpp:602-615

    size_t PointsCount() const { return points_count_; }
    size_t FramesCount() const { return frames_count_; }
    /// EXTENSION (the reference class has no such method): calibrated bundle adjustment from the next ComputeInplace on --
    /// the intrinsics are constants and each frame has the 6 pose variables (srk_ba_set_fixed_intrinsics,
    /// bundle-adj-kanatani.h:113-118).  Throws std::invalid_argument where the library refuses the combination.
    void SetFixedIntrinsics(bool on) {
        int rc = srk_ba_set_fixed_intrinsics(h_, on ? 1 : 0);
        if (rc < 0) Raise(rc);
    }

    /// EXTENSION: robust bundle adjustment from the next ComputeInplace on (srk_ba_set_robust_loss): kind 0 none, 1 Huber,
    /// 2 Cauchy, delta in pixels.  Throws std::invalid_argument for an unknown kind or a delta that is not finite and positive.
    void SetRobustLoss(int kind, Scalar delta) {
        int rc = srk_ba_set_robust_loss(h_, kind, (double)delta);
        if (rc < 0) Raise(rc);
    }

    /// EXTENSION: per-observation information (srk_ba_set_observation_information): q[o] >= 0 multiplies observation o's
    /// squared residual, E = sum rho(q s); one value per observation in the order ComputeInplace flattens them (corner tracks
    /// with a salient point in repository order, inside a track by frame).  An empty vector clears it.  Applied from the next
    /// ComputeInplace on.  Throws std::invalid_argument for a value that is negative or not finite, a count that is not the
    /// resident scene's, or a landmark left with fewer than two observations of positive information.
    void SetObservationInformation(const std::vector<Scalar>& q) {
        int rc = srk_ba_set_observation_information(h_, q.empty() ? nullptr : q.data(), (int64_t)q.size());
        if (rc < 0) Raise(rc);
    }
    /// EXTENSION: the raw residuals in pixels of the last ComputeInplace's result, (x, y) per observation in the same order
    /// (srk_ba_observation_residuals); neither information nor a loss changes them
    std::vector<Scalar> ObservationResiduals() {
        const int64_t size = srk_ba_buffer_size(h_, SRK_BUF_POINT_FRAME); // 3 x frame variables per observation
        if (size < 0) Raise((int)size);
        const int64_t n = size / (3 * (srk_ba_intrinsic_groups(h_) > 0 ? 10 : srk_ba_frame_vars(h_)));
        std::vector<Scalar> e((size_t)(2 * n));
        int rc = srk_ba_observation_residuals(h_, e.data(), n);
        if (rc < 0) Raise(rc);
        return e;
    }

    /// EXTENSION: constant parameter blocks from the next ComputeInplace on (srk_ba_set_constant_blocks).  frame_flags[j] != 0:
    /// frame j keeps its pose (and intrinsics); point_flags[k] != 0: the k-th salient point of the map (the order of
    /// AddSalientPoint) keeps its coordinates -- the adapter maps them to pnt_ind, the order of the tracks that carry a salient
    /// point, the way it maps the points themselves.  Either vector may be empty (none of that kind), both empty clears the
    /// setting.  keep_gauge: the reference's seven gauge variables stay constant as well; false = the constant set alone
    /// fixes the similarity.  Constant entries of the map and of inverse_orient_cams stay bit-identical.  ComputeInplace
    /// throws std::invalid_argument for flag vectors of another size than the map / the cameras, for everything constant,
    /// and where the library refuses the combination (intrinsic groups, more than one rank).
    void SetConstantBlocks(const std::vector<uint8_t>& frame_flags, const std::vector<uint8_t>& point_flags, bool keep_gauge = true) {
        if (frame_flags.empty() && point_flags.empty()) { ClearConstantBlocks(); return; }
        const_frames_ = frame_flags;
        const_points_ = point_flags;
        const_keep_gauge_ = keep_gauge;
        const_set_ = true;
    }
    void ClearConstantBlocks() {
        const_set_ = false;
        const_frames_.clear();
        const_points_.clear();
        int rc = srk_ba_set_constant_blocks(h_, nullptr, 0, nullptr, 0, 1);
        if (rc < 0) Raise(rc);
    }

    /// EXTENSION: Gaussian position priors from the next ComputeInplace on (srk_ba_set_position_priors).
    /// A landmark prior names the k-th salient point of the map (the order of AddSalientPoint) -- the adapter maps it to
    /// pnt_ind, the order of the tracks that carry a salient point, and drops priors on salient points no track carries; a
    /// frame prior names a camera and holds its centre -R^T T.  Positions in the coordinates of the map and the cameras;
    /// info = [xx xy xz yy yz zz], the information matrix in units of the error, (pix / f0)^2, per squared world unit (a prior
    /// of covariance Sigma beside observations of pixel noise sigma_px: (sigma_px / f0)^2 Sigma^-1).  Both vectors empty clears
    /// the setting.  keep_gauge: the reference's seven gauge variables stay constant as well; false = the priors alone fix the
    /// similarity.  ComputeInplace throws std::invalid_argument for an index beyond the map / the cameras, a repeated index,
    /// values the library refuses, and where it refuses the combination (intrinsic groups, more than one rank).
    struct PositionPrior {
        size_t index = 0;
        Point3 position;
        std::array<Scalar, 6> info{};
    };
    void SetPositionPriors(const std::vector<PositionPrior>& point_priors, const std::vector<PositionPrior>& frame_priors, bool keep_gauge = true) {
        if (point_priors.empty() && frame_priors.empty()) { ClearPositionPriors(); return; }
        prior_points_ = point_priors;
        prior_frames_ = frame_priors;
        prior_keep_gauge_ = keep_gauge;
        prior_set_ = true;
    }
    void ClearPositionPriors() {
        prior_set_ = false;
        prior_points_.clear();
        prior_frames_.clear();
        int rc = srk_ba_set_position_priors(h_, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 1);
        if (rc < 0) Raise(rc);
    }

    /// EXTENSION: relative-pose factors between cameras from the next ComputeInplace on (srk_ba_set_relative_pose_factors;
    /// DESIGN.md section 15).  Factor between cameras a != b: rel_R measures R_a R_b^T (row-major, the orientation of camera b
    /// in camera a's frame), rel_t measures R_a (C_b - C_a) (the centre of b in a's frame, world units), info the 21 entries of
    /// the upper triangle of the 6 x 6 information matrix, row by row in the order [t; r], in units of the error, (pix / f0)^2.
    /// Any order: the adapter sorts the factors by (min, max) of their cameras.  An empty vector clears the setting.
    /// ComputeInplace throws std::invalid_argument for a camera beyond the cameras, a pair named twice, values the library
    /// refuses, and where it refuses the combination (intrinsic groups, more than one rank).
    struct RelativePoseFactor {
        size_t frame_a = 0, frame_b = 0;
        std::array<Scalar, 9> rel_R{};
        Point3 rel_t;
        std::array<Scalar, 21> info{};
    };
    void SetRelativePoseFactors(const std::vector<RelativePoseFactor>& factors) {
        if (factors.empty()) { ClearRelativePoseFactors(); return; }
        relpose_ = factors;
        std::stable_sort(relpose_.begin(), relpose_.end(), [](const RelativePoseFactor& x, const RelativePoseFactor& y) {
            const size_t x0 = std::min(x.frame_a, x.frame_b), x1 = std::max(x.frame_a, x.frame_b);
            const size_t y0 = std::min(y.frame_a, y.frame_b), y1 = std::max(y.frame_a, y.frame_b);
            return x0 != y0 ? x0 < y0 : x1 < y1;
        });
    }
    void ClearRelativePoseFactors() {
        relpose_.clear();
        int rc = srk_ba_set_relative_pose_factors(h_, 0, nullptr, nullptr, nullptr, nullptr, nullptr);
        if (rc < 0) Raise(rc);
    }

    /// EXTENSION: marginal covariances of the last ComputeInplace's result (srk_ba_covariances).  frames:
    /// cameras; points: salient points of the map by their place in it (the order of AddSalientPoint) -- the adapter maps them
    /// to pnt_ind as it maps the points themselves.  Any order, repeats allowed.  frame_cov receives one row-major FV x FV block
    /// per camera (FV = 10, or 6 after SetFixedIntrinsics; variable order of bundle-adj-kanatani.h:113-118), point_cov one 3 x 3
    /// block per point, for pixel noise sigma_pixels, in the coordinates of the map and the cameras.  Returns false (outputs
    /// empty) when the undamped system is not positive definite -- with ten variables a frame on planar scenes the intrinsics
    /// are close to unobservable: use SetFixedIntrinsics.  Throws std::invalid_argument for an index beyond the cameras / the
    /// map, a salient point no track of the last ComputeInplace carried, and a sigma that is not finite and positive.
    bool Covariances(const std::vector<size_t>& frames, const std::vector<size_t>& points, Scalar sigma_pixels,
                     std::vector<Scalar>* frame_cov, std::vector<Scalar>* point_cov) {
        std::vector<int32_t> fi;
        std::vector<int64_t> pi;
        for (size_t j : frames) {
            if (j >= frames_count_) throw std::invalid_argument("covariances: a camera index is beyond the cameras");
            fi.push_back((int32_t)j);
        }
        for (size_t k : points) {
            if (k >= pnt_ind_of_.size() || pnt_ind_of_[k] < 0) throw std::invalid_argument("covariances: no track of the last ComputeInplace carries this salient point");
            pi.push_back(pnt_ind_of_[k]);
        }
        const size_t fv = (size_t)srk_ba_frame_vars(h_);
        std::vector<Scalar> fc(fv * fv * fi.size()), pc(9 * pi.size());
        int rc = srk_ba_covariances(h_, (double)sigma_pixels, (int32_t)fi.size(), fi.empty() ? nullptr : fi.data(), fi.empty() ? nullptr : fc.data(),
                                    (int64_t)pi.size(), pi.empty() ? nullptr : pi.data(), pi.empty() ? nullptr : pc.data(), 1);
        if (rc < 0) Raise(rc);
        if (rc != 0) { fc.clear(); pc.clear(); }
        if (frame_cov) *frame_cov = std::move(fc);
        if (point_cov) *point_cov = std::move(pc);
        return rc == 0;
    }
    /// EXTENSION (harness knob): cap a batch of right-hand-side columns of Covariances (srk_ba_set_covariance_batch; 0 = default)
    void SetCovarianceBatch(int64_t max_columns) {
        int rc = srk_ba_set_covariance_batch(h_, max_columns);
        if (rc < 0) Raise(rc);
    }

    /// EXTENSION: cross-covariances between blocks of the last ComputeInplace's result (srk_ba_cross_covariances; DESIGN.md
    /// section 17).  frame_pairs: (camera a, camera b), the block has the rows of a and the columns of b; point_frame_pairs:
    /// (salient point, camera); point_pairs: (salient point, salient point) -- salient points by their place in the map, as in
    /// Covariances.  Any order, repeats allowed, a pair of one block with itself gives its marginal.  ff_cov receives one
    /// row-major FV x FV block per frame pair, pf_cov one 3 x FV block, pp_cov one 3 x 3 block, for pixel noise sigma_pixels, in
    /// the coordinates of the map and the cameras.  Returns false (outputs empty) when the undamped system is not positive
    /// definite.  Throws std::invalid_argument as Covariances does.
    bool CrossCovariances(const std::vector<std::pair<size_t, size_t>>& frame_pairs, const std::vector<std::pair<size_t, size_t>>& point_frame_pairs,
                          const std::vector<std::pair<size_t, size_t>>& point_pairs, Scalar sigma_pixels, std::vector<Scalar>* ff_cov,
                          std::vector<Scalar>* pf_cov, std::vector<Scalar>* pp_cov) {
        const auto frame = [&](size_t j) {
            if (j >= frames_count_) throw std::invalid_argument("cross-covariances: a camera index is beyond the cameras");
            return (int32_t)j;
        };
        const auto point = [&](size_t k) {
            if (k >= pnt_ind_of_.size() || pnt_ind_of_[k] < 0) throw std::invalid_argument("cross-covariances: no track of the last ComputeInplace carries this salient point");
            return (int64_t)pnt_ind_of_[k];
        };
        std::vector<int32_t> fa, fb, pff;
        std::vector<int64_t> pfp, pa, pb;
        for (const auto& x : frame_pairs) { fa.push_back(frame(x.first)); fb.push_back(frame(x.second)); }
        for (const auto& x : point_frame_pairs) { pfp.push_back(point(x.first)); pff.push_back(frame(x.second)); }
        for (const auto& x : point_pairs) { pa.push_back(point(x.first)); pb.push_back(point(x.second)); }
        const size_t fv = (size_t)srk_ba_frame_vars(h_);
        std::vector<Scalar> ff(fv * fv * fa.size()), pf(3 * fv * pfp.size()), pp(9 * pa.size());
        // (an empty vector's data() may be anything; the library wants NULL or a pointer, and reads neither with a count of 0)
        int rc = srk_ba_cross_covariances(h_, (double)sigma_pixels, (int64_t)fa.size(), fa.data(), fb.data(), ff.data(), (int64_t)pfp.size(),
                                          pfp.data(), pff.data(), pf.data(), (int64_t)pa.size(), pa.data(), pb.data(), pp.data(), 1);
        if (rc < 0) Raise(rc);
        if (rc != 0) { ff.clear(); pf.clear(); pp.clear(); }
        if (ff_cov) *ff_cov = std::move(ff);
        if (pf_cov) *pf_cov = std::move(pf);
        if (pp_cov) *pp_cov = std::move(pp);
        return rc == 0;
    }
    /// EXTENSION: the 6 x 6 covariance, order [t; r], of the relative pose z = R_a (C_b - C_a), Z = R_a R_b^T of every pair of
    /// cameras (a, b), a != b, of the last ComputeInplace's result, cross term included (srk_ba_relative_pose_covariances), in the
    /// units of the map and radians: what gates a loop closure.  cov receives one row-major block per pair.  Returns false
    /// (cov empty) when the undamped system is not positive definite.
    bool RelativePoseCovariances(const std::vector<std::pair<size_t, size_t>>& pairs, Scalar sigma_pixels, std::vector<Scalar>* cov) {
        std::vector<int32_t> fa, fb;
        for (const auto& x : pairs) {
            if (x.first >= frames_count_ || x.second >= frames_count_) throw std::invalid_argument("relative-pose covariances: a camera index is beyond the cameras");
            fa.push_back((int32_t)x.first);
            fb.push_back((int32_t)x.second);
        }
        std::vector<Scalar> out(36 * fa.size());
        int rc = srk_ba_relative_pose_covariances(h_, (double)sigma_pixels, (int32_t)fa.size(), fa.data(), fb.data(), out.data());
        if (rc < 0) Raise(rc);
        if (rc != 0) out.clear();
        if (cov) *cov = std::move(out);
        return rc == 0;
    }

    /// EXTENSION: joint Gaussian pose priors over sets of cameras from the next ComputeInplace on
    /// (srk_ba_set_joint_pose_priors): what a marginalised window leaves behind, or with one camera a
    /// full pose prior.  frames: 1 to 16 cameras, strictly ascending; lin_R / lin_C: per camera the linearisation pose, the
    /// world -> camera rotation (row-major) and the centre; mean: 6 values a camera, or empty for zeros; info: the dense
    /// row-major (6 k) x (6 k) information matrix, variable order camera by camera, [t; r] inside a camera, in units of the
    /// error, (pix / f0)^2.  The residual of a camera is [C - lin_C; Log(R^T lin_R)].  keep_gauge = false releases the
    /// reference's gauge: the priors must then fix the seven freedoms.  An empty vector clears the setting.  ComputeInplace
    /// throws std::invalid_argument for a camera beyond the cameras, sizes that do not fit, values the library refuses, and
    /// where it refuses the combination (intrinsic groups, more than one rank).
    struct JointPosePrior {
        std::vector<size_t> frames;
        std::vector<std::array<Scalar, 9>> lin_R;
        std::vector<Point3> lin_C;
        std::vector<Scalar> mean;
        std::vector<Scalar> info;
    };
    void SetJointPosePriors(const std::vector<JointPosePrior>& sets, bool keep_gauge = true) {
        if (sets.empty()) { ClearJointPosePriors(); return; }
        jprior_ = sets;
        jprior_keep_gauge_ = keep_gauge;
    }
    void ClearJointPosePriors() {
        jprior_.clear();
        jprior_keep_gauge_ = true;
        int rc = srk_ba_set_joint_pose_priors(h_, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1);
        if (rc < 0) Raise(rc);
    }

    /// EXTENSION: the prior a sliding window leaves behind, from the last ComputeInplace's result
    /// (srk_ba_marginalization_prior): the cameras `frames` (strictly ascending, at most 8) and the salient
    /// points `points` (by their place in the map, as in Covariances; ascending in the tracks' order) are marginalised, and the
    /// Gaussian that exactly the factors touching them leave on the cameras that stay comes back in information form as a
    /// JointPosePrior over those cameras (numbered as in this scene), linearised at the current poses, with eta (optional) and
    /// the library's report (optional).  Every observation of a dropped camera must belong to a marginalised point.  Returns
    /// false (outputs untouched) when the block of the dropped cameras is not positive definite.  Throws std::invalid_argument
    /// for every refusal of the library and as Covariances does.
    bool MarginalizationPrior(const std::vector<size_t>& frames, const std::vector<size_t>& points, JointPosePrior* prior,
                              std::vector<Scalar>* eta = nullptr, srk_ba_marg_report* report = nullptr) {
        std::vector<int32_t> fi;
        std::vector<int64_t> pi;
        for (size_t j : frames) {
            if (j >= frames_count_) throw std::invalid_argument("marginalization: a camera index is beyond the cameras");
            fi.push_back((int32_t)j);
        }
        for (size_t k : points) {
            if (k >= pnt_ind_of_.size() || pnt_ind_of_[k] < 0) throw std::invalid_argument("marginalization: no track of the last ComputeInplace carries this salient point");
            pi.push_back(pnt_ind_of_[k]);
        }
        std::sort(pi.begin(), pi.end());
        srk_ba_marg_counts cnt{};
        int rc = srk_ba_marginalization_plan(h_, (int32_t)fi.size(), fi.data(), (int64_t)pi.size(), pi.data(), 0, nullptr, &cnt);
        if (rc < 0) Raise(rc);
        const size_t k = (size_t)cnt.n_kept;
        std::vector<int32_t> kept(k + 1);
        std::vector<Scalar> R(9 * k + 1), Cc(3 * k + 1), L(36 * k * k + 1), e(6 * k + 1), m(6 * k + 1);
        int32_t nk = 0;
        srk_ba_marg_report rep{};
        rc = srk_ba_marginalization_prior(h_, (int32_t)fi.size(), fi.data(), (int64_t)pi.size(), pi.data(), (int32_t)k, kept.data(), &nk, R.data(),
                                          Cc.data(), L.data(), e.data(), m.data(), &rep);
        if (rc < 0) Raise(rc);
        if (rc != 0) return false;
        if (prior) {
            prior->frames.assign(kept.begin(), kept.begin() + nk);
            prior->lin_R.resize(k);
            prior->lin_C.resize(k);
            for (size_t q = 0; q < k; ++q) {
                std::copy(R.begin() + 9 * q, R.begin() + 9 * q + 9, prior->lin_R[q].begin());
                prior->lin_C[q] = Point3{ Cc[3 * q], Cc[3 * q + 1], Cc[3 * q + 2] };
            }
            prior->mean.assign(m.begin(), m.begin() + 6 * k);
            prior->info.assign(L.begin(), L.begin() + 36 * k * k);
        }
        if (eta) eta->assign(e.begin(), e.begin() + 6 * k);
        if (report) *report = rep;
        return true;
    }

    /// EXTENSION: new landmarks from corner tracks, on the device (srk_triangulate_tracks / srk_ba_triangulate; DESIGN.md
    /// section 21; the linear system of Triangulate3DPointByLeastSquares, obs-geom.cpp:679-727, solved by a streaming QR
    /// factorisation, with an optional Levenberg-Marquardt refinement of the reprojection error).  One result per track, in
    /// the tracks' order; a track needs no SalientPointId.  status: SRK_TRI_* bits (0 = fine).
    struct TriangulatedPoint {
        Point3 X;
        Scalar rms_pixels = 0, max_ray_angle_deg = 0, cond1 = 0;
        size_t views = 0;
        uint32_t status = 0;
    };
    /// over caller-given cameras (inverse orientations) and intrinsics; an uploaded scene is left untouched.  opts NULL:
    /// the linear result.  Throws std::invalid_argument for every refusal of the library.
    std::vector<TriangulatedPoint> TriangulateTracks(Scalar f0, const std::vector<CornerTrack>& tracks, const std::vector<SE3Transform>& cams,
                                                     const Matrix3* shared_K, const std::vector<Matrix3>* Ks, const srk_tri_options* opts = nullptr) {
        if ((shared_K != nullptr) == (Ks != nullptr)) throw std::invalid_argument("Provide either shared K or separate K for each camera frame");
        if (Ks && Ks->size() != cams.size()) throw std::invalid_argument("triangulate: one K per camera");
        TrackArrays a = FlattenTracks(tracks, cams.size());
        std::vector<Scalar> R, T, K;
        for (const SE3Transform& c : cams) {
            R.insert(R.end(), c.R.begin(), c.R.end());
            T.insert(T.end(), { c.T.x, c.T.y, c.T.z });
        }
        if (shared_K) K.assign(shared_K->begin(), shared_K->end());
        else for (const Matrix3& k : *Ks) K.insert(K.end(), k.begin(), k.end());
        TriOut o(tracks.size());
        int rc = srk_triangulate_tracks(h_, f0, (int64_t)tracks.size(), a.row_ptr.data(), a.frames.data(), a.uv.data(), nullptr, (int32_t)cams.size(),
                                        R.data(), T.data(), K.data(), shared_K ? 1 : 0, opts, o.X.data(), o.q.data(), o.st.data());
        if (rc < 0) Raise(rc);
        return o.Points();
    }
    /// over the CURRENT cameras and intrinsics of the last ComputeInplace's scene, read on the device (after the solve: the
    /// refined ones); the points come back in the coordinates of that call's map.  The scene is not modified.
    std::vector<TriangulatedPoint> Triangulate(const std::vector<CornerTrack>& tracks, const srk_tri_options* opts = nullptr) {
        TrackArrays a = FlattenTracks(tracks, frames_count_);
        TriOut o(tracks.size());
        int rc = srk_ba_triangulate(h_, (int64_t)tracks.size(), a.row_ptr.data(), a.frames.data(), a.uv.data(), nullptr, opts, 1, o.X.data(), o.q.data(),
                                    o.st.data());
        if (rc < 0) Raise(rc);
        return o.Points();
    }

    /// EXTENSION: the poses of frames from 2D-3D correspondences with known landmarks and a predicted pose each, on the device
    /// (srk_resect_frames / srk_ba_resect; DESIGN.md section 22: Levenberg-Marquardt on the reprojection error per frame, with
    /// an optional Huber or Cauchy loss).  One result per frame, in the frames' order.  status: SRK_RESECT_* bits (0 = fine).
    struct ResectObservation {
        size_t point = 0;       ///< index into the landmarks
        Point2f uv;             ///< pixels
        Scalar information = 1; ///< q >= 0; 0 switches the observation off
    };
    struct ResectedFrame {
        SE3Transform pose;                ///< inverse orientation
        Scalar rms_pixels = 0, inlier_share = 0, cond1 = 0, min_depth = 0;
        size_t points = 0, attempts = 0;
        std::array<Scalar, 36> info{};    ///< H / f0^2, row-major: a one-frame set of SetJointPosePriors as it comes
        uint32_t status = 0;
        std::vector<Scalar> weights;      ///< the robust weight of every observation (with want_weights)
    };
    /// over caller-given landmarks; an uploaded scene is left untouched.  opts NULL: the defaults (10 attempts, 1e-9, no loss).
    /// Throws std::invalid_argument for every refusal of the library.
    std::vector<ResectedFrame> ResectFrames(Scalar f0, const std::vector<std::vector<ResectObservation>>& frames, const std::vector<Point3>& landmarks,
                                            const std::vector<SE3Transform>& start, const Matrix3* shared_K, const std::vector<Matrix3>* Ks,
                                            const srk_resect_options* opts = nullptr, bool want_weights = false) {
        ResectArrays a(frames, start, shared_K, Ks, want_weights);
        std::vector<Scalar> X;
        for (const Point3& p : landmarks) X.insert(X.end(), { p.x, p.y, p.z });
        X.push_back(0); // never read: keeps data() valid without landmarks
        int rc = srk_resect_frames(h_, f0, (int32_t)frames.size(), a.row_ptr.data(), a.point.data(), a.uv.data(), a.q.data(), (int64_t)landmarks.size(),
                                   X.data(), a.K.data(), shared_K ? 1 : 0, a.R0.data(), a.T0.data(), opts, a.R.data(), a.T.data(), a.ql.data(),
                                   a.info.data(), a.st.data(), want_weights ? a.w.data() : nullptr);
        if (rc < 0) Raise(rc);
        return a.Frames(want_weights);
    }
    /// over the CURRENT landmarks of the last ComputeInplace's scene, read on the device (after the solve: the refined ones);
    /// point is the landmark's index in that scene (the order of the tracks that have a SalientPointId).  start, the poses and
    /// info are in the coordinates of that call's map.  The scene is not modified.
    std::vector<ResectedFrame> Resect(const std::vector<std::vector<ResectObservation>>& frames, const std::vector<SE3Transform>& start,
                                      const Matrix3* shared_K, const std::vector<Matrix3>* Ks, const srk_resect_options* opts = nullptr,
                                      bool want_weights = false) {
        ResectArrays a(frames, start, shared_K, Ks, want_weights);
        int rc = srk_ba_resect(h_, (int32_t)frames.size(), a.row_ptr.data(), a.point.data(), a.uv.data(), a.q.data(), a.K.data(), shared_K ? 1 : 0,
                               a.R0.data(), a.T0.data(), opts, 1, a.R.data(), a.T.data(), a.ql.data(), a.info.data(), a.st.data(),
                               want_weights ? a.w.data() : nullptr);
        if (rc < 0) Raise(rc);
        return a.Frames(want_weights);
    }

    /// EXTENSION: the poses of frames from 2D-3D correspondences alone, without a predicted pose and with wrong matches among them,
    /// on the device (srk_locate_frames / srk_ba_locate; DESIGN.md section 23: P3P hypotheses from a counter-based sampler, each
    /// scored on every observation, the best one optionally refined by the kernels of ResectFrames).  One result per frame.
    struct LocatedFrame {
        SE3Transform pose;                ///< the located pose, or the refined one with refine (inverse orientation)
        Scalar rms_pixels = 0;            ///< sqrt(score / points) of the truncated score; NaN when not located
        Scalar fourth_point_pixels = 0;   ///< the winning sample's fourth-point error
        size_t points = 0, inlier_count = 0, hypotheses_with_pose = 0;
        int64_t winner = -1;              ///< the winning hypothesis, -1 when not located
        uint32_t located_status = 0;      ///< SRK_LOCATE_* bits (0 = located)
        std::vector<uint8_t> inliers;     ///< per observation, at the located pose (with want_inliers)
        ResectedFrame refined;            ///< the refinement's outputs (with refine)
    };
    /// over caller-given landmarks; an uploaded scene is left untouched.  opts NULL: the defaults (256 hypotheses, 4 px, seed 1);
    /// refine NULL: no refinement.  Throws std::invalid_argument for every refusal of the library.
    std::vector<LocatedFrame> LocateFrames(Scalar f0, const std::vector<std::vector<ResectObservation>>& frames, const std::vector<Point3>& landmarks,
                                           const Matrix3* shared_K, const std::vector<Matrix3>* Ks, const srk_locate_options* opts = nullptr,
                                           const srk_resect_options* refine = nullptr, bool want_inliers = false, bool want_weights = false) {
        ResectArrays a(frames, std::vector<SE3Transform>(frames.size()), shared_K, Ks, want_weights);
        LocateOut o(frames.size(), a.point.size(), want_inliers);
        std::vector<Scalar> X;
        for (const Point3& p : landmarks) X.insert(X.end(), { p.x, p.y, p.z });
        X.push_back(0); // never read: keeps data() valid without landmarks
        int rc = srk_locate_frames(h_, f0, (int32_t)frames.size(), a.row_ptr.data(), a.point.data(), a.uv.data(), a.q.data(), (int64_t)landmarks.size(),
                                   X.data(), a.K.data(), shared_K ? 1 : 0, opts, refine, a.R.data(), a.T.data(), o.located.data(), o.st.data(),
                                   want_inliers ? o.inl.data() : nullptr, a.ql.data(), a.info.data(), a.st.data(), want_weights ? a.w.data() : nullptr);
        if (rc < 0) Raise(rc);
        return o.Frames(a, refine != nullptr, want_inliers, want_weights);
    }
    /// over the CURRENT landmarks of the last ComputeInplace's scene, read on the device; point is the landmark's index in that
    /// scene.  The poses and info are in the coordinates of that call's map.  The scene is not modified.
    std::vector<LocatedFrame> Locate(const std::vector<std::vector<ResectObservation>>& frames, const Matrix3* shared_K, const std::vector<Matrix3>* Ks,
                                     const srk_locate_options* opts = nullptr, const srk_resect_options* refine = nullptr, bool want_inliers = false,
                                     bool want_weights = false) {
        ResectArrays a(frames, std::vector<SE3Transform>(frames.size()), shared_K, Ks, want_weights);
        LocateOut o(frames.size(), a.point.size(), want_inliers);
        int rc = srk_ba_locate(h_, (int32_t)frames.size(), a.row_ptr.data(), a.point.data(), a.uv.data(), a.q.data(), a.K.data(), shared_K ? 1 : 0, opts,
                               refine, 1, a.R.data(), a.T.data(), o.located.data(), o.st.data(), want_inliers ? o.inl.data() : nullptr, a.ql.data(),
                               a.info.data(), a.st.data(), want_weights ? a.w.data() : nullptr);
        if (rc < 0) Raise(rc);
        return o.Frames(a, refine != nullptr, want_inliers, want_weights);
    }

    /// EXTENSION: the relative pose of pairs of images from their 2D-2D matches, wrong matches among them, on the device
    /// (srk_relate_frames; DESIGN.md section 24: five-point hypotheses from a counter-based sampler, each scored on every match by
    /// its Sampson distance; the reference's FindRelativeMotion).  One result per pair: frame a is (I, 0), frame b is `pose` with
    /// x_b ~ R x_a + T and |T| = 1.
    struct Match {
        Point2f a, b;           ///< pixels in the two images
        Scalar information = 1; ///< q >= 0; 0 switches the match off
    };
    struct RelatedPair {
        SE3Transform pose;                ///< (R, T) of frame b; (I, 0) when not related
        std::array<Scalar, 9> E{};        ///< [T]x R, row-major; zero when not related
        Scalar rms_pixels = 0;            ///< sqrt(score / matches) of the truncated score; NaN when not related
        Scalar sixth_match_pixels = 0;    ///< the winning sample's sixth-match Sampson error
        Scalar parallax_rad = 0;          ///< the mean angle between the two rays of the inliers in front of both cameras
        size_t matches = 0, inlier_count = 0, hypotheses_with_model = 0, in_front = 0;
        int64_t winner = -1;              ///< the winning hypothesis, -1 when not related
        uint32_t status = 0;              ///< SRK_RELATE_* bits (0 = related)
        std::vector<uint8_t> inliers;     ///< per match, at the winner (with want_inliers)
    };
    /// shared_Ka / shared_Kb for all pairs, or Kas / Kbs with one matrix per pair.  opts NULL: the defaults (256 hypotheses, 2 px,
    /// seed 1).  An uploaded scene is left untouched.  Throws std::invalid_argument for every refusal of the library.
    std::vector<RelatedPair> RelateFrames(Scalar f0, const std::vector<std::vector<Match>>& pairs, const Matrix3* shared_Ka, const Matrix3* shared_Kb,
                                          const std::vector<Matrix3>* Kas, const std::vector<Matrix3>* Kbs, const srk_relate_options* opts = nullptr,
                                          bool want_inliers = false) {
        const bool shared = shared_Ka && shared_Kb;
        if (shared == (Kas && Kbs) || (!shared && (shared_Ka || shared_Kb)))
            throw std::invalid_argument("Provide either shared intrinsics or separate intrinsics for each pair, for both cameras");
        if (!shared && (Kas->size() != pairs.size() || Kbs->size() != pairs.size())) throw std::invalid_argument("relate: one K_a and one K_b per pair");
        std::vector<int64_t> row_ptr{ 0 };
        std::vector<Scalar> ua, ub, q, Ka, Kb;
        for (const std::vector<Match>& p : pairs) {
            for (const Match& m : p) {
                ua.insert(ua.end(), { m.a.x, m.a.y });
                ub.insert(ub.end(), { m.b.x, m.b.y });
                q.push_back(m.information);
            }
            row_ptr.push_back((int64_t)q.size());
        }
        if (shared) Ka.assign(shared_Ka->begin(), shared_Ka->end()), Kb.assign(shared_Kb->begin(), shared_Kb->end());
        else
            for (size_t i = 0; i < pairs.size(); ++i) {
                Ka.insert(Ka.end(), (*Kas)[i].begin(), (*Kas)[i].end());
                Kb.insert(Kb.end(), (*Kbs)[i].begin(), (*Kbs)[i].end());
            }
        const size_t n = pairs.size(), O = q.size();
        for (std::vector<Scalar>* v : { &ua, &ub, &q, &Ka, &Kb }) v->push_back(0); // never read: keep data() valid without matches or pairs
        std::vector<Scalar> R(9 * n + 1), T(3 * n + 1), E(9 * n + 1), rel(8 * n + 1);
        std::vector<uint32_t> st(n + 1);
        std::vector<uint8_t> inl(want_inliers ? O + 1 : 1);
        int rc = srk_relate_frames(h_, f0, (int32_t)n, row_ptr.data(), ua.data(), ub.data(), q.data(), Ka.data(), Kb.data(), shared ? 1 : 0, opts, R.data(),
                                   T.data(), E.data(), rel.data(), st.data(), want_inliers ? inl.data() : nullptr);
        if (rc < 0) Raise(rc);
        std::vector<RelatedPair> out(n);
        for (size_t i = 0; i < n; ++i) {
            RelatedPair& p = out[i];
            for (size_t e = 0; e < 9; ++e) p.pose.R[e] = R[9 * i + e], p.E[e] = E[9 * i + e];
            p.pose.T = Point3{ T[3 * i], T[3 * i + 1], T[3 * i + 2] };
            p.rms_pixels = rel[8 * i];
            p.matches = (size_t)rel[8 * i + 1];
            p.inlier_count = (size_t)rel[8 * i + 2];
            p.status = st[i];
            p.winner = st[i] ? -1 : (int64_t)rel[8 * i + 3];
            p.hypotheses_with_model = (size_t)rel[8 * i + 4];
            p.sixth_match_pixels = rel[8 * i + 5];
            p.in_front = (size_t)rel[8 * i + 6];
            p.parallax_rad = rel[8 * i + 7];
            if (want_inliers) p.inliers.assign(inl.begin() + row_ptr[i], inl.begin() + row_ptr[i + 1]);
        }
        return out;
    }

    /// EXTENSION: the refinement of two-view poses over all the matches of each pair, on the device (srk_refine_pairs,
    /// srk_relate_frames_refined; DESIGN.md section 26: per pair a Levenberg-Marquardt loop on the robust Sampson error over the five
    /// degrees of freedom of (R, unit T), one wave a pair).  One result per pair.
    struct RefinedPair {
        SE3Transform pose;                ///< (R, T) of frame b, |T| = 1; the start when status has SRK_PAIR_FEW_POINTS
        std::array<Scalar, 9> E{};        ///< [T]x R, row-major
        Scalar rms_pixels = 0;            ///< sqrt(E_pair / matches)
        Scalar mean_weight = 0;           ///< the mean robust weight at the result
        Scalar condition = 0;             ///< cond_1 of the Jacobi-scaled H; large for a pure rotation, NaN when not positive definite
        size_t matches = 0, in_front = 0, attempts = 0;
        std::array<Scalar, 25> info{};    ///< H / f0^2 at the result over [w; beta], row-major
        std::array<Scalar, 6> basis{};    ///< b1, b2: the tangent basis of T that beta refers to
        uint32_t status = 0;              ///< SRK_PAIR_* bits
        std::vector<Scalar> weights;      ///< per match, at the result (with want_weights)
    };
    /// from the start poses `starts` (one per pair; |T| = 1).  opts NULL: the defaults (10 attempts, 1e-9, no loss).  Throws
    /// std::invalid_argument for every refusal of the library.
    std::vector<RefinedPair> RefinePairs(Scalar f0, const std::vector<std::vector<Match>>& pairs, const Matrix3* shared_Ka, const Matrix3* shared_Kb,
                                         const std::vector<Matrix3>* Kas, const std::vector<Matrix3>* Kbs, const std::vector<SE3Transform>& starts,
                                         const srk_pair_options* opts = nullptr, bool want_weights = false) {
        if (starts.size() != pairs.size()) throw std::invalid_argument("pair: one start pose per pair");
        PairArrays a(pairs, shared_Ka, shared_Kb, Kas, Kbs, want_weights);
        std::vector<Scalar> R0(9 * a.n + 1), T0(3 * a.n + 1);
        for (size_t i = 0; i < a.n; ++i) {
            for (size_t e = 0; e < 9; ++e) R0[9 * i + e] = starts[i].R[e];
            T0[3 * i] = starts[i].T.x, T0[3 * i + 1] = starts[i].T.y, T0[3 * i + 2] = starts[i].T.z;
        }
        int rc = srk_refine_pairs(h_, f0, (int32_t)a.n, a.row_ptr.data(), a.ua.data(), a.ub.data(), a.q.data(), a.Ka.data(), a.Kb.data(), a.shared ? 1 : 0,
                                  R0.data(), T0.data(), opts, a.R.data(), a.T.data(), a.E.data(), a.ql.data(), a.info.data(), a.basis.data(), a.st.data(),
                                  want_weights ? a.w.data() : nullptr);
        if (rc < 0) Raise(rc);
        return a.Pairs(want_weights);
    }
    /// RelateFrames with the refinement chained behind it on the device: `related` (may be NULL) receives what RelateFrames returns
    /// except that RelatedPair::pose and RelatedPair::E are the REFINED pose (the C call has one set of pose outputs; the five-point
    /// winner itself is what RelateFrames returns).  refine.inliers_only = 1 refines on the winner's inliers alone.
    std::vector<RefinedPair> RelateFramesRefined(Scalar f0, const std::vector<std::vector<Match>>& pairs, const Matrix3* shared_Ka, const Matrix3* shared_Kb,
                                                 const std::vector<Matrix3>* Kas, const std::vector<Matrix3>* Kbs, const srk_relate_options* opts,
                                                 const srk_pair_options& refine, std::vector<RelatedPair>* related = nullptr, bool want_inliers = false,
                                                 bool want_weights = false) {
        PairArrays a(pairs, shared_Ka, shared_Kb, Kas, Kbs, want_weights);
        std::vector<Scalar> rel(8 * a.n + 1);
        std::vector<uint32_t> rst(a.n + 1);
        std::vector<uint8_t> inl(want_inliers ? a.q.size() : 1);
        int rc = srk_relate_frames_refined(h_, f0, (int32_t)a.n, a.row_ptr.data(), a.ua.data(), a.ub.data(), a.q.data(), a.Ka.data(), a.Kb.data(),
                                           a.shared ? 1 : 0, opts, &refine, a.R.data(), a.T.data(), a.E.data(), rel.data(), rst.data(),
                                           want_inliers ? inl.data() : nullptr, a.ql.data(), a.info.data(), a.basis.data(), a.st.data(),
                                           want_weights ? a.w.data() : nullptr);
        if (rc < 0) Raise(rc);
        std::vector<RefinedPair> out = a.Pairs(want_weights);
        if (related) {
            related->assign(a.n, RelatedPair());
            for (size_t i = 0; i < a.n; ++i) {
                RelatedPair& p = (*related)[i];
                p.pose = out[i].pose;
                p.E = out[i].E;
                p.rms_pixels = rel[8 * i];
                p.matches = (size_t)rel[8 * i + 1];
                p.inlier_count = (size_t)rel[8 * i + 2];
                p.status = rst[i];
                p.winner = rst[i] ? -1 : (int64_t)rel[8 * i + 3];
                p.hypotheses_with_model = (size_t)rel[8 * i + 4];
                p.sixth_match_pixels = rel[8 * i + 5];
                p.in_front = (size_t)rel[8 * i + 6];
                p.parallax_rad = rel[8 * i + 7];
                if (want_inliers) p.inliers.assign(inl.begin() + a.row_ptr[i], inl.begin() + a.row_ptr[i + 1]);
            }
        }
        return out;
    }
    /// The relative-pose factor of a refined pair at a baseline length the caller knows (srk_pair_factor; host only), as
    /// SetRelativePoseFactors takes it for the cameras (frame_a, frame_b): rel_R = R^T, rel_t = -baseline R^T T and the 21
    /// upper-triangle entries of the 6 x 6 information over [t; r].  Its null direction [rel_t; 0] is the scale.
    static RelativePoseFactor PairFactor(const RefinedPair& p, Scalar baseline, size_t frame_a = 0, size_t frame_b = 1) {
        RelativePoseFactor f;
        f.frame_a = frame_a, f.frame_b = frame_b;
        const Scalar T[3] = { p.pose.T.x, p.pose.T.y, p.pose.T.z };
        Scalar R[9], z[3];
        for (size_t e = 0; e < 9; ++e) R[e] = p.pose.R[e];
        if (srk_pair_factor(R, T, p.info.data(), p.basis.data(), baseline, f.rel_R.data(), z, f.info.data()) != SRK_OK)
            throw std::invalid_argument("PairFactor: a value that is not finite, or a baseline <= 0");
        f.rel_t = Point3{ z[0], z[1], z[2] };
        return f;
    }

    /// EXTENSION: the homography p_b ~ G p_a between the matches of pairs of images, wrong matches among them, on the device
    /// (srk_relate_homography; DESIGN.md section 27: four-point hypotheses from a counter-based sampler, each scored on every match
    /// by the symmetric transfer error, the winner refined by Gauss-Newton rounds on its inliers, then decomposed).  The member for
    /// planar scenes and pure rotation, where RelateFrames cannot answer.  One result per pair.
    struct PlanePose {
        SE3Transform pose;  ///< R and T / d (the translation over the plane's distance from camera a)
        Point3 normal;      ///< N in camera a; zero for a pure rotation
        size_t in_front = 0; ///< the inliers with N^T x_a > 0
    };
    struct HomographyPair {
        Matrix3 G{ 1, 0, 0, 0, 1, 0, 0, 0, 1 }; ///< pixels (u, v, f0), Frobenius norm 1; I when there is none
        Matrix3 H{ 1, 0, 0, 0, 1, 0, 0, 0, 1 }; ///< K_b^-1 G K_a over its middle singular value
        std::vector<PlanePose> poses;           ///< none, the rotation alone, or both poses of the plane: the library does not choose
        Scalar rms_pixels = 0;                  ///< sqrt(score / matches) of the truncated score; NaN without a model
        Scalar inlier_rms_pixels = 0;           ///< the RMS symmetric transfer error of the inliers
        Scalar singular_gap = 0;                ///< w1 - w3 of the normalised H^T H; <= 1e-10: a rotation
        size_t matches = 0, inlier_count = 0, hypotheses_with_model = 0, rounds = 0;
        int64_t winner = -1;                    ///< the winning hypothesis, -1 without a model
        uint32_t status = 0;                    ///< SRK_HOMOGRAPHY_* bits (0 = a model)
        std::vector<uint8_t> inliers;           ///< per match, at the returned model (with want_inliers)
    };
    /// shared_Ka / shared_Kb for all pairs, or Kas / Kbs with one matrix per pair.  opts NULL: the defaults (256 hypotheses, 6 px,
    /// seed 1, 4 rounds).  An uploaded scene is left untouched.  Throws std::invalid_argument for every refusal of the library.
    std::vector<HomographyPair> RelateHomography(Scalar f0, const std::vector<std::vector<Match>>& pairs, const Matrix3* shared_Ka, const Matrix3* shared_Kb,
                                                 const std::vector<Matrix3>* Kas, const std::vector<Matrix3>* Kbs,
                                                 const srk_homography_options* opts = nullptr, bool want_inliers = false) {
        PairArrays a(pairs, shared_Ka, shared_Kb, Kas, Kbs, false);
        const size_t n = a.n, O = a.q.size() - 1;
        std::vector<Scalar> G(9 * n + 1), H(9 * n + 1), R(18 * n + 1), T(6 * n + 1), N(6 * n + 1), hg(8 * n + 1);
        std::vector<int32_t> poses(n + 1), front(2 * n + 1);
        std::vector<uint8_t> inl(want_inliers ? O + 1 : 1);
        int rc = srk_relate_homography(h_, f0, (int32_t)n, a.row_ptr.data(), a.ua.data(), a.ub.data(), a.q.data(), a.Ka.data(), a.Kb.data(), a.shared ? 1 : 0,
                                       opts, G.data(), H.data(), poses.data(), R.data(), T.data(), N.data(), front.data(), hg.data(), a.st.data(),
                                       want_inliers ? inl.data() : nullptr);
        if (rc < 0) Raise(rc);
        std::vector<HomographyPair> out(n);
        for (size_t i = 0; i < n; ++i) {
            HomographyPair& p = out[i];
            for (size_t e = 0; e < 9; ++e) p.G[e] = G[9 * i + e], p.H[e] = H[9 * i + e];
            for (int32_t k = 0; k < poses[i]; ++k) {
                PlanePose c;
                for (size_t e = 0; e < 9; ++e) c.pose.R[e] = R[18 * i + 9 * k + e];
                c.pose.T = Point3{ T[6 * i + 3 * k], T[6 * i + 3 * k + 1], T[6 * i + 3 * k + 2] };
                c.normal = Point3{ N[6 * i + 3 * k], N[6 * i + 3 * k + 1], N[6 * i + 3 * k + 2] };
                c.in_front = (size_t)front[2 * i + k];
                p.poses.push_back(c);
            }
            p.rms_pixels = hg[8 * i];
            p.matches = (size_t)hg[8 * i + 1];
            p.inlier_count = (size_t)hg[8 * i + 2];
            p.status = a.st[i];
            p.winner = a.st[i] ? -1 : (int64_t)hg[8 * i + 3];
            p.hypotheses_with_model = (size_t)hg[8 * i + 4];
            p.rounds = (size_t)hg[8 * i + 5];
            p.singular_gap = hg[8 * i + 6];
            p.inlier_rms_pixels = hg[8 * i + 7];
            if (want_inliers) p.inliers.assign(inl.begin() + a.row_ptr[i], inl.begin() + a.row_ptr[i + 1]);
        }
        return out;
    }

    /// EXTENSION: the fundamental matrix p_b^T F p_a = 0 between the matches of pairs of images, wrong matches among them, on the
    /// device and without intrinsics (srk_relate_uncalibrated; DESIGN.md section 28: seven-point hypotheses from a counter-based
    /// sampler, each scored on every match by its Sampson distance, the winner refined by Levenberg-Marquardt attempts over
    /// F = U diag(1, sigma, 0) V^T).  The member for cameras whose K is a guess.  One result per pair.
    struct UncalibratedPair {
        Matrix3 F{};                          ///< pixels (u, v, f0), Frobenius norm 1, rank 2, its largest entry positive; zero without a model
        Matrix3 U{ 1, 0, 0, 0, 1, 0, 0, 0, 1 }; ///< proper rotations with F = U diag(1, sigma, 0) V^T / sqrt(1 + sigma^2)
        Matrix3 V{ 1, 0, 0, 0, 1, 0, 0, 0, 1 };
        Scalar sigma = 0;
        Point3 epipole_a, epipole_b;          ///< the third columns of V and U, homogeneous in (u, v, f0): F e_a = 0, F^T e_b = 0
        std::array<Scalar, 49> information{}; ///< sum q J^T J over the inliers in the order [a; b; delta], pixels^-2
        Scalar rms_pixels = 0;                ///< sqrt(score / matches) of the truncated score; NaN without a model
        Scalar inlier_rms_pixels = 0;         ///< the RMS Sampson distance of the inliers
        Scalar eighth_match_pixels = 0;       ///< the winning sample's eighth-match Sampson error
        Scalar condition = 0;                 ///< cond_1 of the Jacobi-scaled information; NaN when it is not positive definite
        size_t matches = 0, inlier_count = 0, hypotheses_with_model = 0, attempts_accepted = 0, attempts_used = 0, real_roots = 0;
        int64_t winner = -1;                  ///< the winning hypothesis, -1 without a model
        uint32_t status = 0;                  ///< SRK_FUNDAMENTAL_* bits (0 = a model)
        std::vector<uint8_t> inliers;         ///< per match, at the returned model (with want_inliers)
    };
    /// opts NULL: the defaults (256 hypotheses, 2 px, seed 1, 8 attempts).  An uploaded scene is left untouched.  Throws
    /// std::invalid_argument for every refusal of the library.
    std::vector<UncalibratedPair> RelateUncalibrated(Scalar f0, const std::vector<std::vector<Match>>& pairs, const srk_fundamental_options* opts = nullptr,
                                                     bool want_inliers = false) {
        std::vector<int64_t> row_ptr{ 0 };
        std::vector<Scalar> ua, ub, q;
        for (const std::vector<Match>& p : pairs) {
            for (const Match& m : p) {
                ua.insert(ua.end(), { m.a.x, m.a.y });
                ub.insert(ub.end(), { m.b.x, m.b.y });
                q.push_back(m.information);
            }
            row_ptr.push_back((int64_t)q.size());
        }
        const size_t n = pairs.size(), O = q.size();
        for (std::vector<Scalar>* v : { &ua, &ub, &q }) v->push_back(0); // never read: keep data() valid without matches or pairs
        std::vector<Scalar> F(9 * n + 1), U(9 * n + 1), V(9 * n + 1), sg(n + 1), fd(12 * n + 1), info(49 * n + 1);
        std::vector<uint32_t> st(n + 1);
        std::vector<uint8_t> inl(want_inliers ? O + 1 : 1);
        int rc = srk_relate_uncalibrated(h_, f0, (int32_t)n, row_ptr.data(), ua.data(), ub.data(), q.data(), opts, F.data(), U.data(), V.data(), sg.data(),
                                         fd.data(), info.data(), st.data(), want_inliers ? inl.data() : nullptr);
        if (rc < 0) Raise(rc);
        std::vector<UncalibratedPair> out(n);
        for (size_t i = 0; i < n; ++i) {
            UncalibratedPair& p = out[i];
            for (size_t e = 0; e < 9; ++e) p.F[e] = F[9 * i + e], p.U[e] = U[9 * i + e], p.V[e] = V[9 * i + e];
            for (size_t e = 0; e < 49; ++e) p.information[e] = info[49 * i + e];
            p.sigma = sg[i];
            p.epipole_a = Point3{ p.V[2], p.V[5], p.V[8] };
            p.epipole_b = Point3{ p.U[2], p.U[5], p.U[8] };
            p.rms_pixels = fd[12 * i];
            p.matches = (size_t)fd[12 * i + 1];
            p.inlier_count = (size_t)fd[12 * i + 2];
            p.status = st[i];
            p.winner = st[i] ? -1 : (int64_t)fd[12 * i + 3];
            p.hypotheses_with_model = (size_t)fd[12 * i + 4];
            p.eighth_match_pixels = fd[12 * i + 5];
            p.attempts_accepted = (size_t)fd[12 * i + 6];
            p.attempts_used = (size_t)fd[12 * i + 7];
            p.inlier_rms_pixels = fd[12 * i + 8];
            p.condition = fd[12 * i + 10];
            p.real_roots = (size_t)fd[12 * i + 11];
            if (want_inliers) p.inliers.assign(inl.begin() + row_ptr[i], inl.begin() + row_ptr[i + 1]);
        }
        return out;
    }

    /// EXTENSION: the similarity b ~ s R a + t between sets of corresponding 3D points, wrong correspondences among them, on the
    /// device (srk_align_points / srk_ba_align; DESIGN.md section 25: three-point hypotheses from a counter-based sampler, each
    /// scored on every correspondence, the winner refined by a closed-form least-squares similarity on its inliers).  One result
    /// per set.
    struct Correspondence {
        Point3 a, b;            ///< the point in the two maps
        Scalar information = 1; ///< q >= 0; 0 switches the correspondence off
    };
    struct MapCorrespondence {
        size_t point = 0;       ///< the landmark's index in the last ComputeInplace's scene
        Point3 target;          ///< where it lies in the other map
        Scalar information = 1;
    };
    struct AlignedSet {
        Scalar scale = 1;                 ///< s
        Matrix3 R{ 1, 0, 0, 0, 1, 0, 0, 0, 1 };
        Point3 t;                         ///< (1, I, 0) when not aligned
        Scalar rms_distance = 0;          ///< sqrt(score / points) of the truncated score; NaN when not aligned
        Scalar inlier_rms_distance = 0;   ///< the RMS distance of the inliers
        Scalar eigen_gap = 0;             ///< (lambda1 - lambda2) / |lambda1| of the last accepted closed form; NaN without one; 0: collinear inliers
        size_t points = 0, inlier_count = 0, hypotheses_with_model = 0, rounds = 0;
        int64_t winner = -1;              ///< the winning hypothesis, -1 when not aligned
        uint32_t status = 0;              ///< SRK_ALIGN_* bits (0 = aligned)
        std::vector<uint8_t> inliers;     ///< per correspondence, at the returned model (with want_inliers)
    };
    /// over caller-given points; an uploaded scene is left untouched.  opts.inlier_distance must be set (it has no default).
    /// Throws std::invalid_argument with the text of the check for every refusal of the library.
    std::vector<AlignedSet> AlignPoints(const std::vector<std::vector<Correspondence>>& sets, const srk_align_options& opts, bool want_inliers = false) {
        AlignArrays v(sets.size());
        for (const std::vector<Correspondence>& set : sets) {
            for (const Correspondence& c : set) {
                v.a.insert(v.a.end(), { c.a.x, c.a.y, c.a.z });
                v.b.insert(v.b.end(), { c.b.x, c.b.y, c.b.z });
                v.q.push_back(c.information);
            }
            v.row_ptr.push_back((int64_t)v.q.size());
        }
        v.Pad(want_inliers);
        int rc = srk_align_points(h_, (int32_t)sets.size(), v.row_ptr.data(), v.a.data(), v.b.data(), v.q.data(), &opts, v.s.data(), v.R.data(), v.t.data(),
                                  v.al.data(), v.st.data(), want_inliers ? v.inl.data() : nullptr);
        if (rc < 0) Raise(rc);
        return v.Sets(want_inliers);
    }
    /// over the CURRENT landmarks of the last ComputeInplace's scene, read on the device (after the solve: the refined ones); the
    /// similarity maps the coordinates of that call's map to the targets'.  The scene is not modified.
    std::vector<AlignedSet> Align(const std::vector<std::vector<MapCorrespondence>>& sets, const srk_align_options& opts, bool want_inliers = false) {
        AlignArrays v(sets.size());
        for (const std::vector<MapCorrespondence>& set : sets) {
            for (const MapCorrespondence& c : set) {
                if (c.point > 2147483647u) throw std::invalid_argument("align: a landmark index is beyond the map");
                v.point.push_back((int32_t)c.point);
                v.b.insert(v.b.end(), { c.target.x, c.target.y, c.target.z });
                v.q.push_back(c.information);
            }
            v.row_ptr.push_back((int64_t)v.q.size());
        }
        v.Pad(want_inliers);
        int rc = srk_ba_align(h_, (int32_t)sets.size(), v.row_ptr.data(), v.point.data(), v.b.data(), v.q.data(), &opts, 1, v.s.data(), v.R.data(),
                              v.t.data(), v.al.data(), v.st.data(), want_inliers ? v.inl.data() : nullptr);
        if (rc < 0) Raise(rc);
        return v.Sets(want_inliers);
    }
    /// host only: a map under the similarity X' = s R X + t, in place.  Poses are inverse orientations (x_cam = R_c X + T_c): the
    /// camera frame is scaled by s, so every projection is unchanged.  Either group may be NULL.
    static void ApplySimilarity(Scalar s, const Matrix3& R, const Point3& t, std::vector<Point3>* points, std::vector<SE3Transform>* cams) {
        const Scalar tv[3] = { t.x, t.y, t.z };
        std::vector<Scalar> X, cR, cT;
        if (points) for (const Point3& p : *points) X.insert(X.end(), { p.x, p.y, p.z });
        if (cams) for (const SE3Transform& c : *cams) { cR.insert(cR.end(), c.R.begin(), c.R.end()); cT.insert(cT.end(), { c.T.x, c.T.y, c.T.z }); }
        const size_t n = points ? points->size() : 0, m = cams ? cams->size() : 0;
        for (std::vector<Scalar>* v : { &X, &cR, &cT }) v->push_back(0); // never read: keep data() valid
        if (srk_similarity_apply(s, R.data(), tv, (int64_t)n, X.data(), (int64_t)m, cR.data(), cT.data()) < 0)
            throw std::invalid_argument("ApplySimilarity: s must be finite and > 0");
        for (size_t i = 0; i < n; ++i) (*points)[i] = Point3{ X[3 * i], X[3 * i + 1], X[3 * i + 2] };
        for (size_t j = 0; j < m; ++j) {
            for (size_t e = 0; e < 9; ++e) (*cams)[j].R[e] = cR[9 * j + e];
            (*cams)[j].T = Point3{ cT[3 * j], cT[3 * j + 1], cT[3 * j + 2] };
        }
    }

    size_t VarsCount() const { return 3 * points_count_ + (size_t)srk_ba_frame_vars(h_) * frames_count_; }
    size_t NormalizedVarsCount() const { return VarsCount() - 7; }
    const std::string& OptimizationStatusString() const { return status_; }
    const srk_ba_report& Report() const { return report_; }
    /// the C-ABI handle, for callers that also use the srk_mvf_* steps on the same device (the MVF driver)
    srk_ba* Handle() const { return h_; }

private:
    struct TrackArrays {
        std::vector<int64_t> row_ptr{ 0 };
        std::vector<int32_t> frames;
        std::vector<Scalar> uv;
    };
    static TrackArrays FlattenTracks(const std::vector<CornerTrack>& tracks, size_t n_frames) {
        TrackArrays a;
        for (const CornerTrack& t : tracks) {
            for (size_t j = 0; j < n_frames; ++j)
                if (auto c = t.GetCorner(j)) { a.frames.push_back((int32_t)j); a.uv.push_back(c->x); a.uv.push_back(c->y); }
            a.row_ptr.push_back((int64_t)a.frames.size());
        }
        a.frames.push_back(0); // never read: keeps data() valid when no track has a corner
        a.uv.insert(a.uv.end(), { 0, 0 });
        return a;
    }
    struct TriOut {
        std::vector<Scalar> X, q;
        std::vector<uint32_t> st;
        explicit TriOut(size_t n) : X(3 * n + 1), q(4 * n + 1), st(n + 1) {}
        std::vector<TriangulatedPoint> Points() const {
            std::vector<TriangulatedPoint> out(st.size() - 1);
            for (size_t i = 0; i < out.size(); ++i) {
                out[i].X = Point3{ X[3 * i], X[3 * i + 1], X[3 * i + 2] };
                out[i].rms_pixels = q[4 * i];
                out[i].max_ray_angle_deg = q[4 * i + 1];
                out[i].cond1 = q[4 * i + 2];
                out[i].views = (size_t)q[4 * i + 3];
                out[i].status = st[i];
            }
            return out;
        }
    };
    struct PairArrays {
        std::vector<int64_t> row_ptr{ 0 };
        std::vector<Scalar> ua, ub, q, Ka, Kb, R, T, E, ql, info, basis, w;
        std::vector<uint32_t> st;
        size_t n = 0;
        bool shared = false;
        PairArrays(const std::vector<std::vector<Match>>& pairs, const Matrix3* shared_Ka, const Matrix3* shared_Kb, const std::vector<Matrix3>* Kas,
                   const std::vector<Matrix3>* Kbs, bool want_weights) {
            shared = shared_Ka && shared_Kb;
            if (shared == (Kas && Kbs) || (!shared && (shared_Ka || shared_Kb)))
                throw std::invalid_argument("Provide either shared intrinsics or separate intrinsics for each pair, for both cameras");
            if (!shared && (Kas->size() != pairs.size() || Kbs->size() != pairs.size())) throw std::invalid_argument("pair: one K_a and one K_b per pair");
            for (const std::vector<Match>& p : pairs) {
                for (const Match& m : p) {
                    ua.insert(ua.end(), { m.a.x, m.a.y });
                    ub.insert(ub.end(), { m.b.x, m.b.y });
                    q.push_back(m.information);
                }
                row_ptr.push_back((int64_t)q.size());
            }
            if (shared) Ka.assign(shared_Ka->begin(), shared_Ka->end()), Kb.assign(shared_Kb->begin(), shared_Kb->end());
            else
                for (size_t i = 0; i < pairs.size(); ++i) {
                    Ka.insert(Ka.end(), (*Kas)[i].begin(), (*Kas)[i].end());
                    Kb.insert(Kb.end(), (*Kbs)[i].begin(), (*Kbs)[i].end());
                }
            n = pairs.size();
            const size_t O = q.size();
            for (std::vector<Scalar>* v : { &ua, &ub, &q, &Ka, &Kb }) v->push_back(0); // never read: keep data() valid without matches or pairs
            R.resize(9 * n + 1), T.resize(3 * n + 1), E.resize(9 * n + 1), ql.resize(6 * n + 1), info.resize(25 * n + 1), basis.resize(6 * n + 1);
            st.resize(n + 1);
            w.resize(want_weights ? O + 1 : 1);
        }
        std::vector<RefinedPair> Pairs(bool want_weights) const {
            std::vector<RefinedPair> out(n);
            for (size_t i = 0; i < n; ++i) {
                RefinedPair& p = out[i];
                for (size_t e = 0; e < 9; ++e) p.pose.R[e] = R[9 * i + e], p.E[e] = E[9 * i + e];
                p.pose.T = Point3{ T[3 * i], T[3 * i + 1], T[3 * i + 2] };
                p.rms_pixels = ql[6 * i];
                p.matches = (size_t)ql[6 * i + 1];
                p.mean_weight = ql[6 * i + 2];
                p.condition = ql[6 * i + 3];
                p.in_front = ql[6 * i + 4] > 0 ? (size_t)ql[6 * i + 4] : 0; // NaN with FEW_POINTS
                p.attempts = (size_t)ql[6 * i + 5];
                for (size_t e = 0; e < 25; ++e) p.info[e] = info[25 * i + e];
                for (size_t e = 0; e < 6; ++e) p.basis[e] = basis[6 * i + e];
                p.status = st[i];
                if (want_weights) p.weights.assign(w.begin() + row_ptr[i], w.begin() + row_ptr[i + 1]);
            }
            return out;
        }
    };
    struct ResectArrays {
        std::vector<int64_t> row_ptr{ 0 };
        std::vector<int32_t> point;
        std::vector<Scalar> uv, q, K, R0, T0, R, T, ql, info, w;
        std::vector<uint32_t> st;
        ResectArrays(const std::vector<std::vector<ResectObservation>>& frames, const std::vector<SE3Transform>& start, const Matrix3* shared_K,
                     const std::vector<Matrix3>* Ks, bool want_weights) {
            if ((shared_K != nullptr) == (Ks != nullptr)) throw std::invalid_argument("Provide either shared K or separate K for each camera frame");
            if (start.size() != frames.size() || (Ks && Ks->size() != frames.size())) throw std::invalid_argument("resect: one start pose and one K per frame");
            for (const std::vector<ResectObservation>& f : frames) {
                for (const ResectObservation& o : f) {
                    if (o.point > 2147483647u) throw std::invalid_argument("resect: a landmark index is beyond the landmarks");
                    point.push_back((int32_t)o.point);
                    uv.insert(uv.end(), { o.uv.x, o.uv.y });
                    q.push_back(o.information);
                }
                row_ptr.push_back((int64_t)point.size());
            }
            for (const SE3Transform& c : start) {
                R0.insert(R0.end(), c.R.begin(), c.R.end());
                T0.insert(T0.end(), { c.T.x, c.T.y, c.T.z });
            }
            if (shared_K) K.assign(shared_K->begin(), shared_K->end());
            else for (const Matrix3& k : *Ks) K.insert(K.end(), k.begin(), k.end());
            const size_t n = frames.size(), O = point.size();
            point.push_back(0); // never read: keep data() valid without observations or frames
            uv.insert(uv.end(), { 0, 0 });
            q.push_back(0);
            for (std::vector<Scalar>* v : { &K, &R0, &T0 }) v->push_back(0);
            R.resize(9 * n + 1), T.resize(3 * n + 1), ql.resize(6 * n + 1), info.resize(36 * n + 1), st.resize(n + 1);
            w.resize(want_weights ? O + 1 : 1);
        }
        std::vector<ResectedFrame> Frames(bool want_weights) const {
            std::vector<ResectedFrame> out(st.size() - 1);
            for (size_t i = 0; i < out.size(); ++i) {
                ResectedFrame& f = out[i];
                for (size_t e = 0; e < 9; ++e) f.pose.R[e] = R[9 * i + e];
                f.pose.T = Point3{ T[3 * i], T[3 * i + 1], T[3 * i + 2] };
                f.rms_pixels = ql[6 * i];
                f.points = (size_t)ql[6 * i + 1];
                f.inlier_share = ql[6 * i + 2];
                f.cond1 = ql[6 * i + 3];
                f.min_depth = ql[6 * i + 4];
                f.attempts = (size_t)ql[6 * i + 5];
                for (size_t e = 0; e < 36; ++e) f.info[e] = info[36 * i + e];
                f.status = st[i];
                if (want_weights) f.weights.assign(w.begin() + row_ptr[i], w.begin() + row_ptr[i + 1]);
            }
            return out;
        }
    };
    struct LocateOut {
        std::vector<Scalar> located;
        std::vector<uint32_t> st;
        std::vector<uint8_t> inl;
        LocateOut(size_t n, size_t padded_obs, bool want_inliers) : located(6 * n + 1), st(n + 1), inl(want_inliers ? padded_obs : 1) {}
        std::vector<LocatedFrame> Frames(const ResectArrays& a, bool refined, bool want_inliers, bool want_weights) const {
            std::vector<LocatedFrame> out(st.size() - 1);
            std::vector<ResectedFrame> fine;
            if (refined) fine = a.Frames(want_weights);
            for (size_t i = 0; i < out.size(); ++i) {
                LocatedFrame& f = out[i];
                for (size_t e = 0; e < 9; ++e) f.pose.R[e] = a.R[9 * i + e];
                f.pose.T = Point3{ a.T[3 * i], a.T[3 * i + 1], a.T[3 * i + 2] };
                f.rms_pixels = located[6 * i];
                f.points = (size_t)located[6 * i + 1];
                f.inlier_count = (size_t)located[6 * i + 2];
                f.winner = st[i] ? -1 : (int64_t)located[6 * i + 3];
                f.hypotheses_with_pose = (size_t)located[6 * i + 4];
                f.fourth_point_pixels = located[6 * i + 5];
                f.located_status = st[i];
                if (want_inliers) f.inliers.assign(inl.begin() + a.row_ptr[i], inl.begin() + a.row_ptr[i + 1]);
                if (refined) f.refined = fine[i];
            }
            return out;
        }
    };
    struct AlignArrays {
        std::vector<int64_t> row_ptr{ 0 };
        std::vector<int32_t> point;
        std::vector<Scalar> a, b, q, s, R, t, al;
        std::vector<uint32_t> st;
        std::vector<uint8_t> inl;
        explicit AlignArrays(size_t n) : s(n + 1), R(9 * n + 1), t(3 * n + 1), al(8 * n + 1), st(n + 1) {}
        void Pad(bool want_inliers) { // never read: keep data() valid without correspondences or sets
            inl.resize(want_inliers ? q.size() + 1 : 1);
            point.push_back(0);
            for (std::vector<Scalar>* v : { &a, &b, &q }) v->push_back(0);
        }
        std::vector<AlignedSet> Sets(bool want_inliers) const {
            std::vector<AlignedSet> out(st.size() - 1);
            for (size_t i = 0; i < out.size(); ++i) {
                AlignedSet& f = out[i];
                f.scale = s[i];
                for (size_t e = 0; e < 9; ++e) f.R[e] = R[9 * i + e];
                f.t = Point3{ t[3 * i], t[3 * i + 1], t[3 * i + 2] };
                f.rms_distance = al[8 * i];
                f.points = (size_t)al[8 * i + 1];
                f.inlier_count = (size_t)al[8 * i + 2];
                f.status = st[i];
                f.winner = st[i] ? -1 : (int64_t)al[8 * i + 3];
                f.hypotheses_with_model = (size_t)al[8 * i + 4];
                f.rounds = (size_t)al[8 * i + 5];
                f.eigen_gap = al[8 * i + 6];
                f.inlier_rms_distance = al[8 * i + 7];
                if (want_inliers) f.inliers.assign(inl.begin() + row_ptr[i], inl.begin() + row_ptr[i + 1]);
            }
            return out;
        }
    };
    struct Flat {
        std::vector<size_t> ids;
        std::vector<Scalar> pts, R, T, K, uv;
        std::vector<int64_t> row_ptr;
        std::vector<int32_t> frames;
        int shared = 0;
    };
    template <class KVec>
    Flat Flatten(Scalar f0, const FragmentMap& map, const std::vector<SE3Transform>& cams, const CornerTrackRepository& tr,
                 const Matrix3* shared_K, const KVec* Ks) const {
        if (std::fabs(f0) <= 1e-8) throw std::invalid_argument("f0 != 0");                      // .cpp:420
        if ((shared_K != nullptr) == (Ks != nullptr)) throw std::invalid_argument("Provide either shared K or separate K for each camera frame"); // :421
        Flat f;
        f.row_ptr.push_back(0);
        for (const CornerTrack& t : tr.CornerTracks) { // pnt_ind order (:1161-1169)
            if (!t.SalientPointId) continue;
            const Point3& p = map.GetSalientPoint(*t.SalientPointId);
            f.ids.push_back(*t.SalientPointId);
            f.pts.insert(f.pts.end(), { p.x, p.y, p.z });
            for (size_t j = 0; j < cams.size(); ++j)
                if (auto c = t.GetCorner(j)) { f.frames.push_back((int32_t)j); f.uv.push_back(c->x); f.uv.push_back(c->y); }
            f.row_ptr.push_back((int64_t)f.frames.size());
        }
        for (const SE3Transform& c : cams) {
            f.R.insert(f.R.end(), c.R.begin(), c.R.end());
            f.T.insert(f.T.end(), { c.T.x, c.T.y, c.T.z });
        }
        if (shared_K) { f.K.assign(shared_K->begin(), shared_K->end()); f.shared = 1; }
        else for (const Matrix3& k : *Ks) f.K.insert(f.K.end(), k.begin(), k.end());
        return f;
    }
    // the stored flags against this call's scene: points from salient-point order to pnt_ind (f.ids)
    void ApplyConstantBlocks(const FragmentMap& map, const Flat& f, size_t n_frames) {
        if (!const_set_) return;
        if (!const_frames_.empty() && const_frames_.size() != n_frames) throw std::invalid_argument("constant blocks: one frame flag per camera");
        if (!const_points_.empty() && const_points_.size() != map.SalientPointsCount()) throw std::invalid_argument("constant blocks: one point flag per salient point of the map");
        std::vector<uint8_t> pc;
        if (!const_points_.empty()) {
            pc.resize(f.ids.size());
            for (size_t i = 0; i < f.ids.size(); ++i) pc[i] = const_points_.at(map.SalientPointIndex(f.ids[i]));
        }
        int rc = srk_ba_set_constant_blocks(h_, const_frames_.empty() ? nullptr : const_frames_.data(), (int32_t)const_frames_.size(),
                                            const_points_.empty() ? nullptr : pc.data(), (int64_t)pc.size(), const_keep_gauge_ ? 1 : 0);
        if (rc < 0) Raise(rc);
    }
    // the stored priors against this call's scene: landmarks from salient-point order to pnt_ind (f.ids), both kinds ascending
    void ApplyPositionPriors(const FragmentMap& map, const Flat& f) {
        if (!prior_set_) return;
        std::vector<int64_t> at(map.SalientPointsCount(), -1); // salient point -> its prior
        for (size_t k = 0; k < prior_points_.size(); ++k) {
            if (prior_points_[k].index >= at.size()) throw std::invalid_argument("position priors: a landmark index is beyond the map");
            if (at[prior_points_[k].index] >= 0) throw std::invalid_argument("position priors: a landmark is named twice");
            at[prior_points_[k].index] = (int64_t)k;
        }
        std::vector<int64_t> pi;
        std::vector<int32_t> fi;
        std::vector<Scalar> pp, pl, fp, fl;
        auto put = [](const PositionPrior& p, std::vector<Scalar>& pos, std::vector<Scalar>& info) {
            pos.insert(pos.end(), { p.position.x, p.position.y, p.position.z });
            info.insert(info.end(), p.info.begin(), p.info.end());
        };
        for (size_t i = 0; i < f.ids.size(); ++i) {
            const int64_t k = at.at(map.SalientPointIndex(f.ids[i]));
            if (k < 0) continue;
            pi.push_back((int64_t)i);
            put(prior_points_[(size_t)k], pp, pl);
        }
        std::vector<size_t> order(prior_frames_.size());
        for (size_t k = 0; k < order.size(); ++k) order[k] = k;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return prior_frames_[a].index < prior_frames_[b].index; });
        for (size_t k : order) {
            fi.push_back((int32_t)prior_frames_[k].index);
            put(prior_frames_[k], fp, fl);
        }
        int rc = srk_ba_set_position_priors(h_, (int64_t)pi.size(), pi.data(), pp.data(), pl.data(), (int32_t)fi.size(), fi.data(),
                                            fp.data(), fl.data(), prior_keep_gauge_ ? 1 : 0);
        if (rc < 0) Raise(rc);
    }
    // the stored factors, sorted by SetRelativePoseFactors, as the flat arrays of the C ABI
    void ApplyRelativePoseFactors() {
        if (relpose_.empty()) return;
        std::vector<int32_t> fa, fb;
        std::vector<Scalar> R, t, L;
        for (const RelativePoseFactor& f : relpose_) {
            fa.push_back((int32_t)f.frame_a);
            fb.push_back((int32_t)f.frame_b);
            R.insert(R.end(), f.rel_R.begin(), f.rel_R.end());
            t.insert(t.end(), { f.rel_t.x, f.rel_t.y, f.rel_t.z });
            L.insert(L.end(), f.info.begin(), f.info.end());
        }
        int rc = srk_ba_set_relative_pose_factors(h_, (int32_t)fa.size(), fa.data(), fb.data(), R.data(), t.data(), L.data());
        if (rc < 0) Raise(rc);
    }
    // the stored sets as the flat arrays of the C ABI
    void ApplyJointPosePriors() {
        if (jprior_.empty()) return;
        std::vector<int32_t> ptr(1, 0), fr;
        std::vector<Scalar> R, Cc, m, L;
        for (const JointPosePrior& s : jprior_) {
            const size_t k = s.frames.size();
            if (s.lin_R.size() != k || s.lin_C.size() != k || (!s.mean.empty() && s.mean.size() != 6 * k) || s.info.size() != 36 * k * k)
                throw std::invalid_argument("joint pose priors: a set of k cameras needs k poses, 6 k mean values (or none) and (6 k)^2 information entries");
            ptr.push_back(ptr.back() + (int32_t)k);
            for (size_t i = 0; i < k; ++i) {
                fr.push_back((int32_t)s.frames[i]);
                R.insert(R.end(), s.lin_R[i].begin(), s.lin_R[i].end());
                Cc.insert(Cc.end(), { s.lin_C[i].x, s.lin_C[i].y, s.lin_C[i].z });
            }
            if (s.mean.empty()) m.insert(m.end(), 6 * k, Scalar(0));
            else m.insert(m.end(), s.mean.begin(), s.mean.end());
            L.insert(L.end(), s.info.begin(), s.info.end());
        }
        int rc = srk_ba_set_joint_pose_priors(h_, (int32_t)jprior_.size(), ptr.data(), fr.data(), R.data(), Cc.data(), m.data(), L.data(),
                                              jprior_keep_gauge_ ? 1 : 0);
        if (rc < 0) Raise(rc);
    }
    [[noreturn]] void Raise(int rc) const {
        std::string msg = srk_ba_last_error(h_);
        if (rc == SRK_E_ARGS) throw std::invalid_argument(msg);
        throw std::runtime_error("srk_ba: " + msg);
    }
    srk_ba* h_;
    srk_ba_report report_{};
    std::string status_;
    Scalar f0_ = 0;
    size_t points_count_ = 0, frames_count_ = 0;
    bool const_set_ = false, const_keep_gauge_ = true;
    std::vector<uint8_t> const_frames_, const_points_;
    bool prior_set_ = false, prior_keep_gauge_ = true;
    std::vector<PositionPrior> prior_points_, prior_frames_;
    std::vector<RelativePoseFactor> relpose_;
    std::vector<JointPosePrior> jprior_;
    bool jprior_keep_gauge_ = true;
    std::vector<int64_t> pnt_ind_of_;
};

} // namespace suriko_amd
