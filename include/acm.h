/*
 * acm.h -- C-ABI of the MI355X-native batched camera-model engine (libacm.so).
 *
 * Drop-in boundary for the reference's one data-parallel hot path
 * (amin-abouee/apex-camera-models v0.4.1, a pure-Rust crate):
 *
 *   trait CameraModel::project    src/camera/mod.rs:256   (per point, Result)
 *   trait CameraModel::unproject  src/camera/mod.rs:271   (per point, Result)
 *   apex_solver::factors::*CameraParamsFactor  (residual 2N + Jacobian 2N x P,
 *       constructed at bin/camera_converter.rs:378,513,652,794,925,1058)
 *   util::compute_reprojection_error   src/util/error_metrics.rs:62-121
 *   util::sample_points                src/util/point_sampling.rs:46-120
 *
 * Every entry point is batched (a per-point FFI call would be latency bound),
 * takes plain pointers and sizes, never allocates on the hot path, and is
 * stream-ordered on the caller's HIP stream (`void *stream`, NULL = default
 * stream).  All point/ray/residual/Jacobian buffers are DEVICE pointers owned
 * by the caller (hipMalloc'd or from any allocator on the same HIP runtime).
 *
 * Memory layouts (all f64):
 *   points_3d  ACM_LAYOUT_AOS: nalgebra Matrix3xX column-major [x0 y0 z0 x1 ..]
 *              ACM_LAYOUT_SOA: three planes [x0..x(N-1) | y0.. | z0..]
 *   points_2d  nalgebra Matrix2xX column-major [u0 v0 u1 v1 ..]
 *   jacobian   nalgebra DMatrix 2N x P column-major: entry (2i+r, p) at
 *              jacobian[p*2N + 2i + r], r=0 for u, r=1 for v.  Parameter order
 *              is the factor's (camera_converter.rs:385-392, :520-529, ...).
 *   status     one uint8 per point, values acm_point_status below.
 *
 * Return codes: ACM_SUCCESS (0) or a negative acm_result.
 */
#ifndef ACM_H
#define ACM_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define ACM_API __attribute__((visibility("default")))
#else
#define ACM_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* Camera model ids.  Parameter vectors (factor order):
 *   PINHOLE  fx fy cx cy                       (src/camera/pinhole.rs)
 *   RADTAN   fx fy cx cy k1 k2 p1 p2 k3        (src/camera/rad_tan.rs)
 *   KB       fx fy cx cy k1 k2 k3 k4           (src/camera/kannala_brandt.rs)
 *   DS       fx fy cx cy alpha xi              (src/camera/double_sphere.rs)
 *   UCM      fx fy cx cy alpha                 (src/camera/ucm.rs)
 *   EUCM     fx fy cx cy alpha beta            (src/camera/eucm.rs)
 *   FOV      fx fy cx cy w                     (src/camera/fov.rs)          */
typedef enum acm_model {
    ACM_PINHOLE = 0,
    ACM_RADTAN = 1,
    ACM_KANNALA_BRANDT = 2,
    ACM_DOUBLE_SPHERE = 3,
    ACM_UCM = 4,
    ACM_EUCM = 5,
    ACM_FOV = 6
} acm_model;

/* Per-point status, mirroring the CameraModelError variants a projection or
 * unprojection can return (src/camera/mod.rs:80-113). */
typedef enum acm_point_status {
    ACM_STATUS_OK = 0,
    ACM_STATUS_PROJECTION_OUT_SIDE_IMAGE = 1, /* ProjectionOutSideImage */
    ACM_STATUS_POINT_IS_OUT_SIDE_IMAGE = 2,   /* PointIsOutSideImage */
    ACM_STATUS_POINT_AT_CAMERA_CENTER = 3,    /* PointAtCameraCenter */
    ACM_STATUS_NUMERICAL_ERROR = 4            /* NumericalError(_) */
} acm_point_status;

/* Function results.  The positive CameraModelError codes returned by
 * acm_validate_params mirror mod.rs:80-113 variant order + 1. */
typedef enum acm_result {
    ACM_SUCCESS = 0,
    ACM_ERR_INVALID_MODEL = -1,
    ACM_ERR_INVALID_PARAMS = -2, /* CameraModelError::InvalidParams */
    ACM_ERR_INVALID_ARGUMENT = -3,
    ACM_ERR_HIP = -4,
    ACM_ERR_WORKSPACE_TOO_SMALL = -5,
    ACM_ERR_NOT_SUPPORTED = -6,
    ACM_ERR_NUMERICAL = -7 /* CameraModelError::NumericalError */
} acm_result;

typedef enum acm_validation {
    ACM_VALID = 0,
    ACM_FOCAL_LENGTH_MUST_BE_POSITIVE = 4, /* FocalLengthMustBePositive */
    ACM_PRINCIPAL_POINT_MUST_BE_FINITE = 5, /* PrincipalPointMustBeFinite */
    ACM_INVALID_DISTORTION = 6             /* InvalidParams(alpha/xi/beta) */
} acm_validation;

enum { ACM_LAYOUT_AOS = 0, ACM_LAYOUT_SOA = 1 };

/* Per-call option OR-ed into acm_project's `layout`: reference-exact math for
 * Kannala-Brandt and FOV (IEEE sqrt / divisions and a correctly rounded
 * double-double atan2 instead of the fast polynomial / rsq forms, ~1e-16
 * apart).  Projections and Jacobians then equal the reference (Rust f64 +
 * glibc libm) bit for bit wherever glibc's atan2 is correctly rounded, i.e.
 * on all but ~0.2% of arguments, where the two differ by one ulp.  The other
 * five models are reference-exact without it (the flag is ignored). */
enum { ACM_EXACT_MATH = 0x100 };

/* Per-call option OR-ed into acm_unproject's `layout` (and passed in
 * acm_sample_points_ex's `flags`): the reference's own Newton loops for every
 * pixel (kannala_brandt.rs:474-511, rad_tan.rs:436-518) instead of the
 * certified fast ones, and FOV's IEEE unprojection (fov.rs:336-363) instead
 * of its reciprocal / polynomial form.  Statuses (and the sample_points kept
 * set) are identical either way; with the flag RadTan's rays equal the
 * reference's bit for bit (by default they agree within a few ulp).  A
 * per-call choice, so two callers on different threads can use different
 * numerics on the same library (the reference's CameraModel is Send + Sync,
 * mod.rs:241-340).  Replaces the process-wide ACM_TUNE_NEWTON_FAST knob. */
enum { ACM_REFERENCE_NEWTON = 0x200 };

/* Invalid-point policy of the factor evaluation (apex-solver source absent:
 * "skip" matches compute_reprojection_error skipping failed projections,
 * error_metrics.rs:76; "sentinel" is the (1e6,1e6) residual of the removed
 * in-tree factor, doc/COMPREHENSIVE_ANALYSIS.md:116-121).  J = 0 in both. */
enum { ACM_INVALID_SKIP = 0, ACM_INVALID_SENTINEL = 1 };

#define ACM_MAX_PARAMS 9

/* A camera: model id, resolution and the factor-order parameter vector.
 * Replaces the model structs (e.g. KannalaBrandtModel,
 * kannala_brandt.rs:65-72).  Passed by value into every kernel, so the
 * parameters live in SGPRs (uniform across the wave), not in HBM or LDS. */
typedef struct acm_camera {
    int32_t model;
    uint32_t width;
    uint32_t height;
    uint32_t num_params;
    double params[ACM_MAX_PARAMS];
} acm_camera;

/* Number of parameters of a model (Pinhole 4 .. RadTan 9), or -1. */
ACM_API int acm_num_params(int model);

/* Fill *cam.  Mirrors XModel::new(&DVector): wrong parameter count ->
 * ACM_ERR_INVALID_PARAMS (kannala_brandt.rs:122-128, pinhole.rs:60-66, ...).
 * Like the reference, Pinhole and RadTan also run validate_params here
 * (pinhole.rs:80, rad_tan.rs:135): a failure returns ACM_ERR_INVALID_PARAMS.*/
ACM_API int acm_camera_init(acm_camera *cam, int model, const double *params,
                            size_t num_params, uint32_t width, uint32_t height);

/* validate_params (mod.rs:362-371 + per-model rules, e.g.
 * double_sphere.rs:592-607).  Returns an acm_validation code. */
ACM_API int acm_validate_params(const acm_camera *cam);

/* Batched CameraModel::project (+ optional dense parameter Jacobian).
 * points_3d: 3N f64 (layout, optionally | ACM_EXACT_MATH), points_2d: 2N f64
 * out, status: N u8 out,
 * jacobian: 2N*P f64 out or NULL.  Failed points: uv = NaN, J = 0.
 * Replaces mod.rs:256 (per point) and the factor's Jacobian. */
ACM_API int acm_project(const acm_camera *cam, size_t n,
                        const double *points_3d, int layout, double *points_2d,
                        uint8_t *status, double *jacobian, void *stream);

/* The same projection evaluated in f32 (float buffers, same layouts; the
 * camera parameters are rounded to float).  For the f32-vs-f64 tolerance
 * sweep of BASELINE config 5; the reference itself is f64 only.
 *  - points_2d and jacobian are written as float pairs: both must be 8-byte
 *    aligned (points_3d and status need only their own alignment).
 *  - The parameters and the status thresholds are the f64 values rounded to
 *    float: EPS = 2^-52 and sqrt(EPS) = 2^-26 unchanged, 1e-3 as (float)1e-3;
 *    the per-camera constants (DS w2, UCM w, EUCM's (alpha - 1) /
 *    (2 alpha - 1)) are computed in float from the rounded parameters.
 *  - Failed points: uv = NaN, J = 0, as in acm_project.  Every slot of every
 *    output is written, and n = 0 touches nothing.
 *  - Statuses are the exact decision at the rounded inputs wherever binary32
 *    arithmetic in the reference's operation order makes it, i.e. away from
 *    a threshold by more than the rounding of the compared quantity.  An
 *    intermediate beyond FLT_MAX (RadTan's r^6 once |x / z| or |y / z| passes
 *    about 2^21) gives a NaN pixel with status Ok, as the f64 path does at
 *    |x / z| ~ 1e51.
 *  - Accuracy, at the float inputs (tests/f32_ref.py, measured over 26
 *    cameras on an MI355X): |uv - exact| <= 1.7 x 2^-24 S, where S = |c| +
 *    sum |d/dx_k| |x_k| + sum |d/dtheta_q| |theta_q| is the first-order effect
 *    of one relative rounding in every input and parameter (tests allow
 *    11.04).  Jacobian entries within 1 (Pinhole) to 75 (234 at FOV w = 0.2,
 *    whose dw column cancels) x 2^-24 max(|J|, column median), about 2.5 x the
 *    units of 2^-53 the f64 path loses in the same entries. */
ACM_API int acm_project_f32(const acm_camera *cam, size_t n,
                            const float *points_3d, int layout, float *points_2d,
                            uint8_t *status, float *jacobian, void *stream);

/* acm_project plus the derivative with respect to the 3-D POINT: the 2 x 3
 * block d(u, v)/d(x, y, z) per point (basalt's d_proj_d_p3d), what pose
 * refinement, triangulation and bundle adjustment linearise with.
 * points_3d, layout (optionally | ACM_EXACT_MATH), points_2d and status as
 * acm_project, and bit-identical to what acm_project writes for the same
 * arguments.  jacobian_point: 2N x 3 f64 out, column-major like the
 * parameter Jacobian -- entry (2i + r, c) at [c * 2N + 2i + r], r = 0 (u),
 * 1 (v), c = 0, 1, 2 for x, y, z.  Failed points: uv = NaN, J = 0; a point
 * whose status is Ok has a finite block.  Analytic, the derivative of the
 * branch the projection takes: KB at x = y = 0 returns the finite limit
 * [[fx/z, 0, 0], [0, fy/z, 0]]; FOV inside r^2 < 1.49e-8 returns
 * [[fx rd, 0, 0], [0, fy rd, 0]], rd = 2 tan(w/2) / w.  points_2d and
 * jacobian_point must be 16-B aligned (any other offset is fine: every
 * 128-B line of every output stream is stored whole by one workgroup).
 * 89 B per point (24 in, 65 out); no allocation, stream-ordered,
 * reentrant; n = 0 is valid. */
ACM_API int acm_project_point_jacobian(const acm_camera *cam, size_t n,
                                       const double *points_3d, int layout,
                                       double *points_2d, uint8_t *status,
                                       double *jacobian_point, void *stream);

/* Batched CameraModel::unproject (mod.rs:271).  rays: 3N f64 out written in
 * `layout` (optionally | ACM_REFERENCE_NEWTON); failed points: ray = NaN. */
ACM_API int acm_unproject(const acm_camera *cam, size_t n,
                          const double *points_2d, double *rays, int layout,
                          uint8_t *status, void *stream);

/* Factor linearisation: residual r = project(p_i) - obs_i (2N) and the
 * 2N x P Jacobian (nullable) of *CameraParamsFactor
 * (camera_converter.rs:378 & co).  status nullable. */
/* Project -> unproject round trip (BASELINE config 4; the reference's
 * per-point loop of tests/projection_accuracy.rs over mod.rs:256 and :271)
 * in one pass: writes exactly what acm_project (no Jacobian) followed by
 * acm_unproject of its pixels writes -- points_2d (NaN where the projection
 * failed), status, rays (NaN where the unprojection failed) and ray_status
 * -- bit for bit, without reading the pixels back from memory.  layout as
 * acm_project / acm_unproject; with ACM_EXACT_MATH or ACM_REFERENCE_NEWTON
 * set it runs the two calls in order. (r04) */
ACM_API int acm_project_unproject(const acm_camera *cam, size_t n,
                                  const double *points_3d, int layout,
                                  double *points_2d, uint8_t *status,
                                  double *rays, uint8_t *ray_status,
                                  void *stream);
ACM_API int acm_residual_jacobian(const acm_camera *cam, size_t n,
                                  const double *points_3d, int layout,
                                  const double *points_2d_obs,
                                  int invalid_policy, double *residual,
                                  double *jacobian, uint8_t *status,
                                  void *stream);

/* Fused LM linearisation: JtJ (P x P, row-major, symmetric), Jtr (P),
 * cost = 0.5*sum ||r||^2 and n_valid, without materialising r or J.
 * result (device, f64): [JtJ (P*P) | Jtr (P) | cost | n_valid].
 * Deterministic: fixed per-block partials + an ordered final sum.  The
 * workspace (device) must hold acm_normal_equations_workspace_size bytes. */
ACM_API size_t acm_normal_equations_workspace_size(int model, size_t n);
ACM_API int acm_normal_equations(const acm_camera *cam, size_t n,
                                 const double *points_3d, int layout,
                                 const double *points_2d_obs,
                                 int invalid_policy, double *result,
                                 void *workspace, size_t workspace_bytes,
                                 void *stream);

/* compute_reprojection_error (error_metrics.rs:62-121) minus the median:
 * result (device, f64): [rmse, min, max, mean, stddev, n_valid, sum, sumsq]
 * errors (nullable, device, N f64): per-point ||proj - obs||, NaN if failed.
 * The stddev is sum((e - mean)^2) / n (the reference's two-pass form)
 * computed in the same single pass: per-lane shifted sums merged with
 * Chan's pairwise update (equal up to rounding). */
ACM_API size_t acm_reprojection_stats_workspace_size(size_t n);
ACM_API int acm_reprojection_stats(const acm_camera *cam, size_t n,
                                   const double *points_3d, int layout,
                                   const double *points_2d, double *result,
                                   double *errors, void *workspace,
                                   size_t workspace_bytes, void *stream);
/* compute_reprojection_error (error_metrics.rs:62-121) in full, one call:
 * result (device, 9 f64) = acm_reprojection_stats' 8 + [8] the median of the
 * valid errors (acm_median_valid's rule; NaN when n_valid = 0).  The
 * statistics pass also counts the median's first radix-select histogram
 * (per workgroup, merged afterwards), so the median reads the errors one
 * time fewer than acm_reprojection_stats + acm_median_valid, and n_valid
 * stays on the device in between.  errors: nullable device N f64 output
 * (NaN if failed); when NULL they live in the workspace. */
ACM_API size_t acm_reprojection_error_workspace_size(size_t n);
ACM_API int acm_reprojection_error(const acm_camera *cam, size_t n,
                                   const double *points_3d, int layout,
                                   const double *points_2d, double *result,
                                   double *errors, void *workspace,
                                   size_t workspace_bytes, void *stream);
/* Host-side merge of the results of disjoint shards (the multi-GPU form of
 * compute_reprojection_error, error_metrics.rs:86-111): parts = nparts x 8
 * host doubles, each an acm_reprojection_stats result, folded in order --
 * sums added, extrema combined, (n_valid, mean, n * stddev^2) merged by
 * Chan's pairwise update -- into result (8 host doubles, same layout).  One
 * all-gather of the 8 doubles per rank + this merge gives every rank the
 * same statistics bit for bit.  A point whose error is NaN (failed
 * projection or NaN observation) is never counted. */
ACM_API int acm_reprojection_stats_merge(size_t nparts, const double *parts, double *result);

/* The same 8-double result from an error vector already in HBM (errors:
 * device, N f64, NaN = invalid; e.g. a shard's acm_reprojection_stats
 * `errors` output): the per-shard leg of the multi-GPU statistics
 * (error_metrics.rs:86-111 over one shard) without copying the errors to the
 * host.  Same per-workgroup shifted sums + fixed-order Chan merge as
 * acm_reprojection_stats, so bit-reproducible run to run. */
ACM_API size_t acm_error_stats_workspace_size(size_t n);
ACM_API int acm_error_stats(size_t n, const double *errors, double *result,
                            void *workspace, size_t workspace_bytes, void *stream);

/* linear_estimation (kannala_brandt.rs:164-272, double_sphere.rs:225-290,
 * ucm.rs:200-258, eucm.rs:216-288, rad_tan.rs:153-234).  The 2N x k system
 * [A | b] is never materialised: acm_linear_system_qr reduces its rows on
 * the GPU into the (k+1)x(k+1) upper-triangular R factor of a tall-skinny QR
 * (r_factor: device, packed row-major upper triangle; error_flag: device int,
 * set on the reference's NumericalError path).  acm_linear_estimation then
 * solves R_A x = z on the host with nalgebra's SVD::solve(eps) semantics
 * (eps = f64::EPSILON for KB, 1e-10 otherwise), applies the model's clamps
 * and validation, and writes the estimate into cam->params (k = 4 KB,
 * 3 RadTan, 1 DS/UCM/EUCM; FOV: the grid search below). */
ACM_API int acm_linear_system_columns(int model);
ACM_API size_t acm_linear_system_qr_workspace_size(int model, size_t n);
ACM_API int acm_linear_system_qr(const acm_camera *cam, size_t n,
                                 const double *points_3d, int layout,
                                 const double *points_2d, double *r_factor,
                                 int *error_flag, void *workspace,
                                 size_t workspace_bytes, void *stream);
ACM_API size_t acm_linear_estimation_workspace_size(int model, size_t n);
/* convert_to_*'s opening (camera_converter.rs:371-375): the reprojection
 * error of *cam as given (initial_error; device, 9 f64 as
 * acm_reprojection_error) and then linear_estimation of *cam (updated in
 * place, return code as acm_linear_estimation) -- for the TSQR models in ONE
 * pass over the correspondences (k_tsqr also computes the errors, their
 * statistics and the median's first histogram).  The initial error is
 * written even when the estimation then fails (as the reference computes it
 * first); for FOV and too-few-point calls the two run one after the other. */
ACM_API size_t acm_linear_estimation_with_error_workspace_size(int model, size_t n);
ACM_API int acm_linear_estimation_with_error(acm_camera *cam, size_t n,
                                             const double *points_3d, int layout,
                                             const double *points_2d,
                                             double *initial_error, void *workspace,
                                             size_t workspace_bytes, void *stream);
/* (r05) The same, returning as soon as *cam is estimated: the initial
 * error's 8 statistics (acm_reprojection_stats' layout, n_valid at [5]) are
 * copied to initial_error_host (nullable, host, 8 f64) before the median
 * runs, the host solve overlaps the median, and the median itself lands in
 * initial_error[8] in stream order (read it after a later synchronisation of
 * `stream`; the workspace must stay allocated until then).  What
 * conversion.convert uses, so the LM's first evaluation queues behind the
 * median without a host round trip in between.  acm_linear_estimation_with_error
 * is this call followed by a synchronisation of `stream`. */
ACM_API int acm_linear_estimation_with_error_async(acm_camera *cam, size_t n,
                                                   const double *points_3d, int layout,
                                                   const double *points_2d,
                                                   double *initial_error,
                                                   double *initial_error_host, void *workspace,
                                                   size_t workspace_bytes, void *stream);
/* Multi-GPU linear_estimation: each rank runs acm_linear_system_qr on its
 * shard, the packed factors (host copies) are folded in rank order with
 * acm_linear_system_r_merge (Givens; R of the stacked rows), error flags
 * OR-ed, and acm_linear_estimation_solve finishes on every rank with the
 * global point count.  acm_linear_estimation = qr + solve on one GPU. */
ACM_API int acm_linear_system_r_merge(int model, double *r_inout,
                                      const double *r_other);
ACM_API int acm_linear_estimation_solve(acm_camera *cam, size_t n_total,
                                        const double *r_factor_host,
                                        int error_flag);
ACM_API int acm_linear_estimation(acm_camera *cam, size_t n,
                                  const double *points_3d, int layout,
                                  const double *points_2d, void *workspace,
                                  size_t workspace_bytes, void *stream);

/* FOV linear_estimation (fov.rs:153-251) is a grid search, not a linear
 * system: for w = i/100, i = 10..299 (ACM_FOV_GRID_SIZE values) the sum of
 * finite reprojection errors and their count over all points.
 * acm_fov_grid_errors writes grid_sums (device, 2 x 290 doubles: the 290
 * error sums, then the 290 counts); the sums are additive over shards of
 * the points, so a multi-GPU caller all-reduces them before
 * acm_fov_grid_select, which keeps the first w with the strictly smallest
 * mean (host array), applies the clamp to [0.01, 3] and validate_params,
 * and writes w into cam->params[4].  acm_linear_estimation runs both for
 * ACM_FOV (n < 2 -> ACM_ERR_INVALID_PARAMS, fov.rs:166-171). */
#define ACM_FOV_GRID_SIZE 290
ACM_API size_t acm_fov_grid_workspace_size(size_t n);
ACM_API int acm_fov_grid_errors(const acm_camera *cam, size_t n,
                                const double *points_3d, int layout,
                                const double *points_2d, double *grid_sums,
                                void *workspace, size_t workspace_bytes,
                                void *stream);
ACM_API int acm_fov_grid_select(acm_camera *cam, const double *grid_sums_host);

/* Bounded Levenberg-Marquardt over the fused normal equations: the
 * apex-solver call of camera_converter.rs:381-420.  Each evaluation runs
 * acm_normal_equations, then (if allreduce != NULL) hands the device result
 * vector [JtJ | Jtr | cost | n_valid] to the callback for a cross-rank sum
 * (e.g. RCCL all-reduce), copies it to the host and solves the damped
 * P x P system by Cholesky.  cam->params: initial value in, optimum out. */
typedef struct acm_lm_config {
    int32_t max_iterations;      /* 100 (camera_converter.rs:411) */
    int32_t invalid_policy;      /* ACM_INVALID_SKIP / _SENTINEL */
    double cost_tolerance;       /* 1e-6 relative cost decrease */
    double parameter_tolerance;  /* 1e-8 */
    double gradient_tolerance;   /* 1e-6 on |Jtr|_inf */
    double initial_damping;      /* mu0 (Marquardt-scaled), 1e-4 */
    uint32_t has_bounds;
    uint32_t reserved;
    double lower[ACM_MAX_PARAMS]; /* set_variable_bounds */
    double upper[ACM_MAX_PARAMS];
} acm_lm_config;

enum {
    ACM_LM_MAX_ITERATIONS = 0,
    ACM_LM_COST = 1,
    ACM_LM_PARAMETER = 2,
    ACM_LM_GRADIENT = 3,
    ACM_LM_FAILED = 4
};

typedef struct acm_lm_summary {
    int32_t iterations;
    int32_t termination; /* ACM_LM_* */
    int32_t evaluations;
    int32_t reserved;
    double initial_cost; /* 0.5 * sum ||r||^2 */
    double final_cost;
    double n_valid;
} acm_lm_summary;

typedef int (*acm_allreduce_fn)(void *ctx, double *device_buffer, size_t count,
                                void *stream);

/* (r06) Grid-sampled correspondences by cell (acm_sample_points_cells):
 * cell c = i * num_cells_x + j of the row-major grid whose centres are
 * ((j + 0.5) * (width / num_cells_x), (i + 0.5) * (height / num_cells_y))
 * -- the f64 cell size first, then the product, each rounded once
 * (point_sampling.rs:56-78; width, height: the SAMPLED camera's
 * resolution).  A uint32 per point instead of the 16-B pixel: the cell
 * forms below recompute each pixel exactly as sample_points wrote it, so
 * their results are the pixel forms' bit for bit (with the default
 * ACM_TUNE_NE_WAVES / NE_UNROLL, which they always use). */
typedef struct acm_cell_grid {
    uint32_t num_cells_x, num_cells_y;
    uint32_t width, height;
} acm_cell_grid;
ACM_API int acm_normal_equations_cells(const acm_camera *cam, size_t n,
                                       const double *points_3d, int layout,
                                       const uint32_t *cells, const acm_cell_grid *grid,
                                       int invalid_policy, double *result, void *workspace,
                                       size_t workspace_bytes, void *stream);

ACM_API void acm_lm_default_config(acm_lm_config *cfg);
ACM_API size_t acm_lm_workspace_size(int model, size_t n);
ACM_API int acm_lm_optimize(acm_camera *cam, size_t n, const double *points_3d,
                            int layout, const double *points_2d,
                            const acm_lm_config *cfg, acm_allreduce_fn allreduce,
                            void *allreduce_ctx, acm_lm_summary *summary,
                            void *workspace, size_t workspace_bytes, void *stream);
/* (r06) acm_lm_optimize over cell-form observations (acm_cell_grid):
 * the same iterates, 12 B per point less read per evaluation.  Workspace:
 * acm_lm_workspace_size. */
ACM_API int acm_lm_optimize_cells(acm_camera *cam, size_t n, const double *points_3d,
                                  int layout, const uint32_t *cells,
                                  const acm_cell_grid *grid, const acm_lm_config *cfg,
                                  acm_allreduce_fn allreduce, void *allreduce_ctx,
                                  acm_lm_summary *summary, void *workspace,
                                  size_t workspace_bytes, void *stream);
/* (r06) The conversion's other two passes in the cell form, the same bits:
 * acm_reprojection_error over cell-form observations (workspace:
 * acm_reprojection_error_workspace_size), and
 * acm_linear_estimation_with_error_async whose fused pass reads the cells
 * (points_2d still required: the FOV grid search and the too-few-points
 * path read pixels; workspace: acm_linear_estimation_with_error_workspace_size). */
ACM_API int acm_reprojection_error_cells(const acm_camera *cam, size_t n,
                                         const double *points_3d, int layout,
                                         const uint32_t *cells, const acm_cell_grid *grid,
                                         double *result, double *errors, void *workspace,
                                         size_t workspace_bytes, void *stream);
ACM_API int acm_linear_estimation_with_error_cells_async(
    acm_camera *cam, size_t n, const double *points_3d, int layout, const double *points_2d,
    const uint32_t *cells, const acm_cell_grid *grid, double *initial_error,
    double *initial_error_host, void *workspace, size_t workspace_bytes, void *stream);

/* Camera pose refinement (PnP refinement): the camera is fixed, the unknown
 * is the rigid transform world -> camera, p_cam = R p_world + t.  r is the
 * rotation matrix, row-major.  The perturbation is delta = (rho_x rho_y
 * rho_z phi_x phi_y phi_z), applied on the left:
 *   acm_pose_retract (host only):  R <- Exp(phi) R,  t <- Exp(phi) t + rho,
 * Exp = Rodrigues' formula (a series for |phi|^2 < 1e-6, half-angle forms
 * beyond: nothing cancels).
 * acm_pose_normal_equations: per point p = R X + t, r = project(p) - obs,
 * J = Jpoint(p) [ I | -[p]x ] (2 x 6), accumulated without materialising
 * r, J or p.  result (device, 44 f64): [JtJ (6 x 6, row-major, symmetric) |
 * Jtr (6) | cost = 0.5 sum ||r||^2 | n_valid] -- acm_normal_equations'
 * layout with P = 6.  Points whose projection is not Ok, or whose
 * observation is NaN, are skipped and not counted.  Deterministic (fixed
 * per-workgroup partials + an ordered final sum: repeated calls return the
 * same bits); 40 B per point read.  layout: ACM_LAYOUT_AOS / _SOA only.
 * workspace (device): acm_pose_normal_equations_workspace_size bytes.
 * acm_pose_optimize: acm_lm_optimize's state machine with P = 6 in local
 * coordinates -- each trial step h is evaluated at retract(pose, h), and the
 * pose moves when the step is accepted.  *pose: start in, optimum out.
 * cfg->has_bounds != 0 is ACM_ERR_INVALID_ARGUMENT (a local perturbation has
 * no box); cfg->invalid_policy is ignored (invalid points are skipped).
 * allreduce (nullable) receives the 44-double device vector of every
 * evaluation.  workspace (device): acm_pose_optimize_workspace_size bytes. */
typedef struct acm_pose {
    double r[9];
    double t[3];
} acm_pose;
ACM_API int acm_pose_retract(acm_pose *pose, const double delta[6]);
ACM_API size_t acm_pose_normal_equations_workspace_size(size_t n);
ACM_API int acm_pose_normal_equations(const acm_camera *cam, const acm_pose *pose, size_t n,
                                      const double *points_world, int layout,
                                      const double *points_2d_obs, double *result,
                                      void *workspace, size_t workspace_bytes, void *stream);
ACM_API size_t acm_pose_optimize_workspace_size(size_t n);
ACM_API int acm_pose_optimize(const acm_camera *cam, acm_pose *pose, size_t n,
                              const double *points_world, int layout,
                              const double *points_2d_obs, const acm_lm_config *cfg,
                              acm_allreduce_fn allreduce, void *allreduce_ctx,
                              acm_lm_summary *summary, void *workspace,
                              size_t workspace_bytes, void *stream);

/* Batched multi-view triangulation: the dual of pose refinement -- the
 * poses (world -> camera, p_cam = R X + t) are known, the unknowns are the
 * 3-D points, one independent 3 x 3 problem per point.  One camera
 * (intrinsics) serves all views; a rig with different intrinsics per view is
 * out of scope.
 *
 * Tracks are CSR: point i owns observations track_offsets[i] ..
 * track_offsets[i + 1] - 1, in that order (track_offsets: n_points + 1
 * entries, non-decreasing, [0] = 0, the last <= n_observations; entries
 * outside [0, n_observations] are clamped, so no offset can make the call
 * read out of bounds).  Observation j is the pixel obs_uv[2 j], obs_uv[2 j + 1]
 * seen through poses[obs_view[j]].
 *
 * Midpoint start (skipped with ACM_TRI_USE_INITIAL, which starts from
 * points_world as given).  An observation is usable iff its pixel is finite,
 * its view index lies in [0, n_views) and the unprojection of the pixel
 * (acm_unproject's default numerics) is Ok; anything else is skipped -- an
 * out-of-range view index is never dereferenced and is no error of the call.
 * Per usable observation d = R^T ray, c = -R^T t; A = sum (I - d d^T),
 * b = sum (I - d d^T) c, in track order.  Fewer than 2 usable observations:
 * ACM_TRI_TOO_FEW_OBSERVATIONS.  det(A) < 2 min_parallax_sin2 (tr(A) / 4)^3:
 * ACM_TRI_DEGENERATE (for two rays at angle phi this reads sin^2 phi <
 * min_parallax_sin2).  Otherwise X0 = A^-1 b.  (UCM's start inherits the
 * reference's 1 - r^2 unprojection quirk; the refinement removes
 * it.)
 *
 * Refinement: minimise sum ||project(R X + t) - uv||^2 (the fast projection
 * of acm_pose_normal_equations) over the observations whose pixel is finite,
 * whose view is in range and whose projection at the current X is Ok; their
 * count is n_valid.  Per observation J = Jpoint(p) R (2 x 3); sums in track
 * order.  The loop is acm_lm_optimize's state machine with P = 3 and no
 * bounds (Marquardt-scaled damping with the same floor, Nielsen update, a
 * failed Cholesky raises the damping, the same three tolerances, damping >
 * 1e32 fails, one evaluation per trial step), plus one rule: a trial step
 * whose n_valid is smaller than the current one's is rejected (a two-view
 * point must not lower its cost by losing an observation).  Fewer than 2
 * valid observations at the start point: ACM_TRI_TOO_FEW_OBSERVATIONS.  A
 * tolerance ends the loop: ACM_TRI_OK.  The iteration limit or a failure:
 * ACM_TRI_NOT_CONVERGED, with the best accepted X written.  max_iterations
 * = 0: the start point, ACM_TRI_OK, cost / n_valid / information evaluated
 * there.
 *
 * Outputs per point: points_world (3 f64, AoS; in/out with
 * ACM_TRI_USE_INITIAL), status (acm_tri_status), and when non-NULL cost
 * (0.5 sum ||r||^2 at the returned X), n_valid, information (the upper
 * triangle of the undamped J^T J at the returned X, row by row: xx xy xz yy
 * yz zz).  ACM_TRI_TOO_FEW_OBSERVATIONS and ACM_TRI_DEGENERATE write X = NaN,
 * cost = NaN, information = 0 and n_valid = the count that decided (usable
 * observations of the start, or valid ones at the start point).
 *
 * A point's outputs depend only on its own observation list in order, the
 * poses, the camera and the config -- not on n_points, its index, its
 * neighbours or the launch: the same track gives the same bits anywhere in
 * any batch.  One lane per point; each wave stages the contiguous run of its
 * 64 tracks' observations in LDS once (20 B each) when the run holds at most
 * ACM_TRI_STAGE_OBSERVATIONS of them, and reads global memory per evaluation
 * otherwise (the same arithmetic in the same order).
 *
 * Errors: NULL cam / poses / track_offsets / cfg / points_world / status, or
 * NULL obs_view / obs_uv with n_observations > 0, negative max_iterations or
 * unknown flag bits: ACM_ERR_INVALID_ARGUMENT; a bad model:
 * ACM_ERR_INVALID_MODEL; a NULL or short workspace (device,
 * acm_triangulate_workspace_size bytes): ACM_ERR_WORKSPACE_TOO_SMALL.
 * n_points = 0 is valid and touches nothing.  Stream-ordered, no allocation,
 * reentrant. */
typedef enum acm_tri_status {
    ACM_TRI_OK = 0,
    ACM_TRI_TOO_FEW_OBSERVATIONS = 1, /* fewer than 2 usable observations */
    ACM_TRI_DEGENERATE = 2,           /* rays (nearly) parallel: no depth */
    ACM_TRI_NOT_CONVERGED = 3         /* iteration limit or damping overflow; X still written */
} acm_tri_status;

enum { ACM_TRI_USE_INITIAL = 1 };     /* start from points_world as given, skip the midpoint start */

/* observations a wave stages in LDS (20 B each); a longer run is read from
 * global memory at every evaluation */
#define ACM_TRI_STAGE_OBSERVATIONS 512

typedef struct acm_triangulate_config {
    int32_t max_iterations;      /* per point; 0 = midpoint start only.  default 20 */
    int32_t flags;               /* 0 or ACM_TRI_USE_INITIAL */
    double cost_tolerance;       /* defaults of acm_lm_default_config: 1e-6 */
    double parameter_tolerance;  /* 1e-8 */
    double gradient_tolerance;   /* 1e-6 */
    double initial_damping;      /* 1e-4 */
    double min_parallax_sin2;    /* degeneracy threshold, above.  default 1e-8 */
} acm_triangulate_config;

ACM_API void acm_triangulate_default_config(acm_triangulate_config *cfg);
ACM_API size_t acm_triangulate_workspace_size(size_t n_points, size_t n_observations);
ACM_API int acm_triangulate(const acm_camera *cam, size_t n_views, const acm_pose *poses,
                            size_t n_points, const int64_t *track_offsets,
                            size_t n_observations, const int32_t *obs_view,
                            const double *obs_uv, const acm_triangulate_config *cfg,
                            double *points_world, uint8_t *status, double *cost,
                            uint32_t *n_valid, double *information, void *workspace,
                            size_t workspace_bytes, void *stream);

/* Batched pose refinement: the dual of acm_triangulate -- the world points
 * are known, the unknowns are the poses (world -> camera, p_cam = R X + t),
 * one independent 6 x 6 problem per view, all views in one launch with the
 * Levenberg-Marquardt loop on the device.  One camera (intrinsics) serves all
 * views.  Together with acm_triangulate this is an alternating bundle
 * adjustment with no host round trip.
 *
 * poses: n_views acm_pose, in/out.  points_world: 3 n_points f64, AoS, read
 * only.  Observations are CSR by view: view k owns observations
 * view_offsets[k] .. view_offsets[k + 1] - 1, in that order (view_offsets:
 * n_views + 1 entries; entries outside [0, n_observations] are clamped as
 * acm_triangulate clamps its offsets, so no offset can make the call read
 * out of bounds).  Observation j is the pixel obs_uv[2 j], obs_uv[2 j + 1] of
 * world point obs_point[j].
 *
 * An observation is valid iff its pixel is finite, obs_point[j] lies in
 * [0, n_points), the world point is finite (acm_triangulate writes NaN for
 * the points it could not solve; this call takes its output as it is) and
 * the projection of R X + t (the fast projection of
 * acm_pose_normal_equations) is Ok at the pose being evaluated; anything else
 * is skipped -- an out-of-range index is never dereferenced and is no error
 * of the call.  The count of valid observations is n_valid.
 *
 * Per view the problem is acm_pose_optimize's: r = project(p) - uv,
 * J = Jp [I | -[p]x], left perturbation delta = (rho, phi), R <- Exp(phi) R,
 * t <- Exp(phi) t + rho (acm_pose_retract's formulas, in double on the
 * device), acm_lm_optimize's state machine with P = 6 and no bounds in local
 * coordinates: the same damping, update, tolerances and constants.  A
 * tolerance ends the loop: ACM_POSE_OK.  The iteration limit, a non-finite
 * start cost or damping > 1e32: ACM_POSE_NOT_CONVERGED, with the best
 * accepted pose written.  Fewer than 3 valid observations at the start pose:
 * ACM_POSE_TOO_FEW_OBSERVATIONS, the pose left as given bit for bit, cost =
 * NaN, information = 0, iterations = 0, n_valid = the count.  max_iterations
 * = 0: the pose unchanged bit for bit, ACM_POSE_OK, cost / n_valid /
 * information evaluated there.
 *
 * Outputs per view: poses, status (acm_pose_status, required), and when
 * non-NULL cost (0.5 sum ||r||^2 at the returned pose), n_valid, iterations,
 * information (the 21 upper-triangle entries of the undamped J^T J at the
 * returned pose, row by row, parameters in the order rho, phi).
 *
 * A view's outputs depend only on its own observation list in order, the
 * world points those observations name, its start pose, the camera and the
 * config -- not on n_views, its index, the other views or the launch: the
 * same view gives the same bits anywhere in any batch, and repeated calls
 * return the same bits.  One 256-lane workgroup per view; a view with at
 * most ACM_POSE_BATCH_STAGE_OBSERVATIONS observations stages them (pixel and
 * gathered point, 40 B each) in LDS once, a longer one gathers from global
 * memory at every evaluation (the same arithmetic in the same order).  Only
 * n_views workgroups run; measured down to 8 views of 5000 observations the
 * call is still 7x faster than one acm_pose_optimize per view, and a few
 * views far longer than that (where acm_pose_optimize spreads one view over
 * the whole device) were not measured.  The default
 * of 20 iterations is acm_triangulate's, not acm_lm_default_config's 100.
 *
 * Errors: NULL cam / poses / view_offsets / cfg / status, NULL points_world
 * with n_points > 0, NULL obs_point / obs_uv with n_observations > 0,
 * negative max_iterations or nonzero flags: ACM_ERR_INVALID_ARGUMENT; a bad
 * model: ACM_ERR_INVALID_MODEL; a NULL or short workspace (device,
 * acm_pose_optimize_batch_workspace_size bytes): ACM_ERR_WORKSPACE_TOO_SMALL.
 * n_views = 0 is valid and touches nothing.  Stream-ordered, no allocation,
 * no host synchronisation, reentrant. */
typedef enum acm_pose_status {
    ACM_POSE_OK = 0,
    ACM_POSE_TOO_FEW_OBSERVATIONS = 1, /* fewer than 3 valid observations at the start pose */
    ACM_POSE_NOT_CONVERGED = 2         /* iteration limit or damping overflow; best accepted pose written */
} acm_pose_status;

/* observations of one view staged in LDS (40 B each); a longer view is read
 * from global memory at every evaluation */
#define ACM_POSE_BATCH_STAGE_OBSERVATIONS 1024

typedef struct acm_pose_batch_config {
    int32_t max_iterations;      /* per view; 0 = evaluate only.  default 20 */
    int32_t flags;               /* must be 0 */
    double cost_tolerance;       /* defaults of acm_lm_default_config: 1e-6 */
    double parameter_tolerance;  /* 1e-8 */
    double gradient_tolerance;   /* 1e-6 */
    double initial_damping;      /* 1e-4 */
} acm_pose_batch_config;

ACM_API void acm_pose_optimize_batch_default_config(acm_pose_batch_config *cfg);
ACM_API size_t acm_pose_optimize_batch_workspace_size(size_t n_views, size_t n_observations);
ACM_API int acm_pose_optimize_batch(const acm_camera *cam, size_t n_views, acm_pose *poses,
                                    size_t n_points, const double *points_world,
                                    const int64_t *view_offsets, size_t n_observations,
                                    const int32_t *obs_point, const double *obs_uv,
                                    const acm_pose_batch_config *cfg, uint8_t *status,
                                    double *cost, uint32_t *n_valid, int32_t *iterations,
                                    double *information, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* Absolute pose from scratch: the minimal solver and RANSAC over it.  Every
 * solver above is a local Levenberg-Marquardt that needs a start pose and
 * takes every observation at face value; these two calls produce that start
 * pose from raw 2-D / 3-D correspondences, and the set of observations that
 * agree with it.  The camera models are mostly omnidirectional, so the solver
 * works on bearing vectors (unprojected rays), not on normalised pixels.
 *
 * acm_p3p: n independent triplets, one lane each.  bearings: 9 n f64, triplet
 * i holds f1, f2, f3 (they need not be unit; the call normalises them);
 * points_world: 9 n f64, X1, X2, X3.  poses: 4 n acm_pose; count: n bytes.
 * A solution is a pose (world -> camera, p = R X + t) for which R X_i + t is a
 * positive multiple of f_i, i = 1, 2, 3.  All real solutions with positive
 * depths are returned, count[i] in 0 .. 4 of them in poses[4 i ..], in the
 * order of the quartic's roots below; the slots beyond count[i] are NaN.  R is
 * a rotation (orthonormal to rounding, det +1) by construction.
 *
 * The route is Grunert's, in f64: with a = |X2 - X3|, b = |X1 - X3|, c =
 * |X1 - X2| and the cosines of the angles between the bearings, a quartic in
 * v = s3 / s1 (s_i the depths); the quartic (or, when its constant term is the
 * larger, the one in 1 / v) is factored into two real quadratics through the
 * largest real root of its resolvent cubic -- no eigen-solver -- and each real
 * root takes two Newton steps on the quartic; u = s2 / s1 follows from a
 * linear relation and s1 from the law of cosines; v <= 0 or u <= 0 is dropped.
 * The depths then take three Gauss-Newton steps on the three law-of-cosines
 * equations, and a solution is kept when its depths are positive and the
 * three residuals are at most 1e-12 (a^2 + b^2 + c^2).  R, t align the
 * orthonormal frame of (s_i f_i) -- first axis along the first edge, third
 * the triangle's normal -- to the frame of (X_i), and the centroids.  A
 * (numerically) double root of the quartic may be returned twice.
 *
 * count = 0: a non-finite input, a bearing without direction, collinear or
 * repeated world points, or two parallel bearings (the sine of the angle at
 * most 1e-10 in each case), or no real solution.  n = 0 is valid.  NULL
 * buffers with n > 0: ACM_ERR_INVALID_ARGUMENT.  No workspace, stream-ordered,
 * reentrant.
 *
 * acm_pose_estimate_batch: RANSAC over that solver, one 256-lane workgroup per
 * view, all views in one launch.  The input is acm_pose_optimize_batch's (CSR
 * by view, view_offsets clamped into [0, n_observations], one camera for all
 * views) without start poses: poses is output only.
 *
 * An observation is usable iff its pixel is finite, obs_point[j] lies in
 * [0, n_points), its world point is finite and the unprojection of the pixel
 * (acm_unproject's default numerics, as acm_triangulate's midpoint start) is
 * Ok with a finite direction; its bearing f is that ray, normalised.  Three
 * models differ, each because the unprojection keeps a behaviour of the
 * reference under which its ray is not the one that projects to the pixel; in
 * each that unprojection still decides Ok and f is the projection's inverse.
 * UCM: the unprojection's denominator is 1 - r^2 (off by up to 1.5e-2 rad on
 * the sample camera; no pose fits such bearings); f is the same formula with
 * 1 + r^2.
 * FOV: the unprojection divides by cos(rd w), rd = |m|, which is negative
 * beyond 90 degrees (rd w > pi / 2) and makes its normalised ray the antipode
 * of the true one; f = (mx s / (rd 2 tan(w/2)), my s / (rd 2 tan(w/2)), c),
 * (s, c) = sincos(rd w), normalised: the same ray wherever c > 0, continuous
 * through 90 degrees, z < 0 beyond.  A pixel with rd w >= pi is the image of
 * no ray: not usable.  (On the axis, rd <= sqrt(eps), and for 2 tan(w/2) <=
 * sqrt(eps) f is the unprojection's ray.)
 * KB: the unprojection clamps ru = |m| to pi / 2 and solves theta_d(theta) =
 * pi / 2 for every pixel beyond (58 px off in the sample camera's corners),
 * and stops its Newton iteration at |delta| < 1e-6 (up to 5e-11 rad under
 * strong distortion); f = (mx sin(theta) / ru, my sin(theta) / ru,
 * cos(theta)) with theta from the same iteration on theta_d(theta) = ru
 * unclamped (from theta = ru, at most 10 steps, until |delta| < 1e-6) and one
 * more step.  A pixel for which that iteration does not converge is not
 * usable.  (ru <= 1e-6: the unprojection's ray.)
 * RadTan's ray is the unprojection's, which ends its Newton iteration at a
 * residual of 1e-6: up to 1e-6 rad (6e-4 px) from the true direction here;
 * the two-view solvers polish it (acm_relative_pose_batch).
 * Anything else is skipped -- an out-of-range index is never dereferenced and
 * is no error of the call.  n_usable (nullable) receives the count per view.
 * The view's records (X, Y, Z, fx, fy, fz; 48 B) are built once: in LDS for a
 * view of at most ACM_POSE_EST_STAGE_OBSERVATIONS observations, in the
 * workspace otherwise (the same arithmetic in the same order), so an
 * iterative unprojection (KB, RadTan) runs once per observation, never per
 * hypothesis.
 *
 * Hypothesis h = 0 .. n_hypotheses - 1 (lanes stride over h) draws local
 * indices j = (splitmix64(seed + ctr 0x9E3779B97F4A7C15) cnt) >> 64 with ctr =
 * 8 h + d + 1 for the draws d = 0 .. 7, cnt the view's (clamped) observation
 * count, all in 64-bit wrapping arithmetic and splitmix64(z): z = (z ^ z >>
 * 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) 0x94D049BB133111EB; z ^ z >> 31.
 * The first three draws that are usable and pairwise distinct form the
 * sample; if eight draws do not yield three the hypothesis is void.  The draw
 * depends on seed, h and cnt only.  The sample goes through acm_p3p's solver,
 * and each of its solutions is scored over all usable observations of the
 * view in order: with p = R X + t, observation j is an inlier iff f.p > 0 and
 * (f.p)^2 >= cos^2(inlier_angle) (p.p).  The key of a solution is (inlier
 * count descending, sum over the inliers of 1 - (f.p)^2 / (p.p) ascending, h
 * ascending, solution index ascending), a total order, so the winner does not
 * depend on the order of the reduction.
 *
 * Outputs per view: the winner's pose, status (acm_pose_est_status, required),
 * n_inliers (required), and when non-NULL inlier_mask (one byte per
 * observation, 1 for the winner's inliers, 0 for every other entry of the
 * view's clamped range, unusable observations included).  Fewer than 4 usable
 * observations: ACM_POSE_EST_TOO_FEW_OBSERVATIONS, the pose all NaN, n_inliers
 * = 0, the mask 0.  No hypothesis with a solution, or a best count below
 * min_inliers: ACM_POSE_EST_NO_MODEL, the pose NaN, n_inliers = the best count
 * (0 without a model), the mask 0.  Views whose clamped ranges overlap (which
 * valid offsets never do) write the same mask bytes from several workgroups.
 *
 * A view's outputs depend only on its own observation list in order, the
 * points it names, the camera and the config -- not on n_views, its index or
 * the other views -- and repeated calls return the same bits.
 *
 * Errors: acm_pose_optimize_batch's list (n_inliers is required like status;
 * workspace: device, 8-byte aligned, acm_pose_estimate_batch_workspace_size
 * bytes), and ACM_ERR_INVALID_ARGUMENT for n_hypotheses outside 1 .. 65536,
 * nonzero flags, inlier_angle outside (0, pi/2) or min_inliers < 4.  n_views =
 * 0 is valid and touches nothing.  Stream-ordered, no allocation, no host
 * synchronisation, reentrant (two calls in flight need two workspaces). */
ACM_API int acm_p3p(size_t n, const double *bearings, const double *points_world,
                    acm_pose *poses, uint8_t *count, void *stream);

typedef enum acm_pose_est_status {
    ACM_POSE_EST_OK = 0,
    ACM_POSE_EST_TOO_FEW_OBSERVATIONS = 1, /* fewer than 4 usable observations */
    ACM_POSE_EST_NO_MODEL = 2              /* no solution, or fewer than min_inliers inliers */
} acm_pose_est_status;

/* observations of one view whose records stay in LDS (48 B each); a longer
 * view keeps them in the workspace */
#define ACM_POSE_EST_STAGE_OBSERVATIONS 1024

typedef struct acm_pose_estimate_config {
    int32_t n_hypotheses;   /* default 256; 1 .. 65536 */
    int32_t flags;          /* must be 0 */
    uint64_t seed;          /* default 1 */
    double inlier_angle;    /* radians, in (0, pi/2); default 5e-3 */
    int32_t min_inliers;    /* default 4; >= 4 */
    int32_t reserved;
} acm_pose_estimate_config;

ACM_API void acm_pose_estimate_batch_default_config(acm_pose_estimate_config *cfg);
ACM_API size_t acm_pose_estimate_batch_workspace_size(size_t n_views, size_t n_observations);
ACM_API int acm_pose_estimate_batch(const acm_camera *cam, size_t n_views, acm_pose *poses,
                                    size_t n_points, const double *points_world,
                                    const int64_t *view_offsets, size_t n_observations,
                                    const int32_t *obs_point, const double *obs_uv,
                                    const acm_pose_estimate_config *cfg, uint8_t *status,
                                    uint32_t *n_inliers, uint8_t *inlier_mask,
                                    uint32_t *n_usable, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* Two-view relative pose: the 8-point solver and RANSAC over it.  Everything
 * above needs a pose or known 3-D points from outside; these two calls produce
 * the pose of camera B relative to camera A from 2-D / 2-D matches alone, and
 * the set of matches that agree with it, so acm_triangulate can start from two
 * images of an unknown scene.  Convention for both: p_b = R p_a + t with
 * |t| = 1 (the scale is unobservable), E = [t]x R and f_b^T E f_a = 0 for the
 * bearings f_a, f_b of a match; the output is an acm_pose.  The solver works
 * on bearing vectors, not on normalised pixels, because most of the models are
 * omnidirectional.
 *
 * acm_relative_pose_8pt: n independent problems of eight matches, one lane
 * each.  bearings_a, bearings_b: 24 n f64, problem i holds its eight bearings
 * in image A and in image B (any length; the call normalises them).  poses: n
 * acm_pose; essential (nullable): 9 n f64, E row-major with unit Frobenius
 * norm, signed as [t]x R; n_front: n bytes, the number of the eight matches in
 * front of both cameras of the returned pose.
 *
 * The route, f64 throughout, works for any row count >= 8 (the refit below
 * reuses it).  Match i gives the row a = f_b (x) f_a (nine entries, E
 * row-major, so a . vec(E) = f_b^T E f_a).  The rows are streamed through
 * Givens rotations into a 9 x 9 upper-triangular factor R9 -- no pivoting, no
 * normal equations (A^T A squares the conditioning: its Cholesky route lost
 * two digits in the median and had a tail of gross errors) -- and a diagonal
 * entry with |r_kk| < 2^-60 max |R9| is replaced by that value with its sign
 * (with eight rows the last entry is exactly 0).  The null vector is the
 * smallest right singular vector of R9 by three rounds of inverse iteration
 * on R9^T R9 (solve R9^T z = x, normalise, solve R9 y = z, normalise) from
 * x0 ~ (1, 2, ..., 9); no component is fixed to 1, so motions with zeros in E
 * (forward: a zero row; sideways: a zero diagonal) work.  E is decomposed in
 * closed form, without an SVD (Horn 1990): B = tr(E E^T) / 2 I - E E^T = b b^T
 * gives b as B's column of the largest diagonal entry over the root of that
 * entry; with C the matrix of the rows e2 x e3, e3 x e1, e1 x e2 of E's rows,
 * R+- = (C -+ [b]x E) / (b . b), each made a rotation by Gram-Schmidt on rows
 * 0 and 1 and the cross product as row 2.  The four candidates are, in order,
 * (R+, b^), (R+, -b^), (R-, -b^), (R-, b^).  A match is in front of both
 * cameras iff, with g = R f_a and c = g . f_b, c (f_b . t) - g . t > 0 and
 * (f_b . t) - c (g . t) > 0 (no division); the candidate with the most rows in
 * front wins, the first of equals.
 *
 * A non-finite input, a bearing without direction or a non-finite result: the
 * pose and the essential matrix all NaN, n_front = 0.  Degenerate inputs --
 * rows whose null space has dimension >= 2: repeated matches, all points on
 * one plane, pure rotation -- return some member of that null space with no
 * guarantee; the RANSAC below discards them by their score.  n = 0 is valid.
 * NULL buffers (essential excepted) with n > 0: ACM_ERR_INVALID_ARGUMENT.  No
 * workspace, stream-ordered, reentrant.
 *
 * acm_relative_pose_batch: RANSAC over that solver, one 256-lane workgroup per
 * view pair, all pairs in one launch.  Matches are CSR by pair: pair k owns
 * the matches pair_offsets[k] .. pair_offsets[k + 1] - 1 (offsets clamped
 * into [0, n_matches] as acm_pose_estimate_batch clamps its own), uv_a and
 * uv_b (2 n_matches f64 each) their pixels in image A and in image B.  One
 * camera serves both images of every pair.
 *
 * A match is usable iff both pixels are finite and both unprojections
 * (acm_unproject's default numerics) are Ok with a finite direction; its
 * bearings are those rays, normalised, with four exceptions in which that
 * unprojection still decides Ok: for UCM, FOV and KB the bearing is the
 * projection's inverse, and a FOV pixel with rd w >= pi or a KB pixel whose
 * Newton iteration does not converge is not usable, all as
 * acm_pose_estimate_batch documents; for RadTan, whose
 * unprojection ends its Newton iteration once the distortion residual is
 * below 1e-6 and so misses the direction that projects to the pixel by up to
 * 1e-6 rad (an exact pair of 8 matches finds no model with such rays at a
 * 1e-6 rad threshold), the bearing is that ray after two more steps of the
 * same iteration.  n_usable (nullable) receives the count
 * per pair.  The pair's records (f_a, f_b; 48 B) are built once: in LDS for a
 * pair of at most ACM_RELPOSE_STAGE_MATCHES matches, in the workspace
 * otherwise (the same arithmetic in the same order), so an iterative
 * unprojection (KB, RadTan) runs twice per match, never per hypothesis.
 *
 * Hypothesis h = 0 .. n_hypotheses - 1 (lanes stride over h) draws local
 * indices with acm_pose_estimate_batch's splitmix64 and ctr = 16 h + d + 1
 * for the draws d = 0 .. 15.  The first eight draws that are usable and
 * pairwise distinct form the sample; if sixteen draws do not yield eight the
 * hypothesis is void.  The sample goes through the solver above (cheirality
 * over its eight matches) and the pose is scored over all usable matches of
 * the pair in order: with g = R f_a, n = t x g and d = f_b . n, a match is an
 * inlier iff n . n > 0, d^2 <= sin^2(inlier_angle) (n . n) -- f_b lies within
 * inlier_angle of the epipolar plane -- and both cheirality expressions above
 * are positive.  A match without parallax carries no depth sign and is not
 * counted.  The key of a hypothesis is (inlier count descending, sum over the
 * inliers of d^2 / (n . n) ascending, h ascending), a total order, so the
 * winner does not depend on the order of the reduction.
 *
 * Refit.  A minimal sample of noisy matches is a weak estimate, so when the
 * winner has at least min_inliers inliers, up to refit_rounds times the
 * workgroup streams the rows of the current model's inliers into R9 -- lane l
 * takes the matches l, l + 256, ... in order, the 64 factors of a wave are
 * merged by a fixed butterfly (one factor's rows are fed into the other),
 * then the four waves' in order, so the result depends on nothing but the
 * match list -- runs the solver on that factor (cheirality over those
 * inliers) and scores the result over all usable matches.  It replaces the
 * current model iff its (count descending, score ascending) is strictly
 * better; otherwise, or when the solve fails, the loop ends.
 *
 * Outputs per pair: the pose, status (acm_relpose_status, required),
 * n_inliers (required) and, when non-NULL, inlier_mask (one byte per match, 1
 * for the final model's inliers, 0 for every other entry of the pair's
 * clamped range, unusable matches included).  Fewer than 8 usable matches:
 * ACM_RELPOSE_TOO_FEW_MATCHES, the pose all NaN, n_inliers = 0, the mask 0.
 * No hypothesis with a finite model, or a best count below min_inliers (the
 * refit is not tried then): ACM_RELPOSE_NO_MODEL, the pose NaN, n_inliers =
 * the best count (0 without a model), the mask 0.  Pairs whose clamped ranges
 * overlap (which valid offsets never do) write the same mask bytes and
 * workspace records from several workgroups.
 *
 * A pair's outputs depend only on its own match list in order, the camera and
 * the config -- not on n_pairs, its index or the other pairs -- and repeated
 * calls return the same bits.
 *
 * Errors: acm_pose_estimate_batch's list (workspace: device, 8-byte aligned,
 * acm_relative_pose_batch_workspace_size bytes), and ACM_ERR_INVALID_ARGUMENT
 * for n_hypotheses outside 1 .. 65536, nonzero flags, inlier_angle outside
 * (0, pi/2), min_inliers < 8 or refit_rounds outside 0 .. 8.  n_pairs = 0 is
 * valid and touches nothing.  Stream-ordered, no allocation, no host
 * synchronisation, reentrant (two calls in flight need two workspaces).
 *
 * Out of scope: a 5-point minimal solver (it survives planar scenes and needs
 * 5 instead of 8 clean matches per sample, but its 10 x 20 elimination and
 * degree-10 root finding do not fit a lane's registers); pure rotation and
 * planar scenes, whose model is the homography of acm_homography_4pt and
 * acm_homography_batch below (their inlier count and tau beside this call's
 * count are what a choice between the two models needs; the choice itself is
 * the caller's); a non-linear refinement of E; two different cameras per
 * pair; spreading one pair's hypotheses over several workgroups. */
ACM_API int acm_relative_pose_8pt(size_t n, const double *bearings_a, const double *bearings_b,
                                  acm_pose *poses, double *essential, uint8_t *n_front,
                                  void *stream);

typedef enum acm_relpose_status {
    ACM_RELPOSE_OK = 0,
    ACM_RELPOSE_TOO_FEW_MATCHES = 1, /* fewer than 8 usable matches */
    ACM_RELPOSE_NO_MODEL = 2         /* no finite model, or fewer than min_inliers inliers */
} acm_relpose_status;

/* matches of one pair whose records stay in LDS (48 B each); a longer pair
 * keeps them in the workspace */
#define ACM_RELPOSE_STAGE_MATCHES 1024

typedef struct acm_relative_pose_config {
    int32_t n_hypotheses;   /* default 512; 1 .. 65536 */
    int32_t flags;          /* must be 0 */
    uint64_t seed;          /* default 1 */
    double inlier_angle;    /* radians, in (0, pi/2); default 5e-3 */
    int32_t min_inliers;    /* default 8; >= 8 */
    int32_t refit_rounds;   /* default 3; 0 .. 8 */
} acm_relative_pose_config;

ACM_API void acm_relative_pose_batch_default_config(acm_relative_pose_config *cfg);
ACM_API size_t acm_relative_pose_batch_workspace_size(size_t n_pairs, size_t n_matches);
ACM_API int acm_relative_pose_batch(const acm_camera *cam, size_t n_pairs, acm_pose *poses,
                                    const int64_t *pair_offsets, size_t n_matches,
                                    const double *uv_a, const double *uv_b,
                                    const acm_relative_pose_config *cfg, uint8_t *status,
                                    uint32_t *n_inliers, uint8_t *inlier_mask,
                                    uint32_t *n_usable, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* Two-view homography: the 4-point solver and RANSAC over it.  When all
 * matches lie on one plane, or camera B only rotates, the 8-point system above
 * loses rank; the model of exactly those two cases is f_b ~ H f_a for the
 * bearings of a match, H = R + (t / d) n^T with the plane n . X = d > 0 in
 * camera A's frame (n a unit vector) and the motion p_b = R p_a + t.  Like the
 * calls above these work on bearing vectors and serve all seven models.
 *
 * acm_homography_4pt: n independent problems of four matches, one lane each.
 * bearings_a, bearings_b: 12 n f64, problem i holds its four bearings in image
 * A and in image B (any length; the call normalises them).  Outputs per
 * problem: homography, 9 f64, H row-major with its middle singular value 1 and
 * f_b . (H f_a) > 0 for the majority of the four matches; count, one byte, the
 * number of solutions 0, 1 or 2; poses, two acm_pose, the motion of each
 * solution with t scaled to unit length (acm_relative_pose_*'s convention);
 * planes, 2 x 4 f64, (n_x, n_y, n_z, d / |t|) of each solution; translation
 * (nullable), one f64, tau = sigma_1 - sigma_3 = |t| / d, the baseline over the
 * plane's distance; n_front, two bytes, per solution the number of the four
 * matches with n . f_a > 0.  The slots beyond count are NaN (n_front 0).
 *
 * The route, f64 throughout, works for any match count >= 4 (the refit below
 * reuses it).  Match i gives the three rows [f_b]x (x) f_a, so that the rows
 * times vec(H) are f_b x (H f_a); all three are fed, because for an
 * omnidirectional bearing no fixed one is redundant.  They go through the
 * Givens factor R9 and the inverse-iteration null vector of
 * acm_relative_pose_8pt.  The eigenpairs lambda_1 >= lambda_2 >= lambda_3, v_1,
 * v_2, v_3 of the symmetric H^T H come from a cyclic Jacobi of six sweeps; H is
 * divided by sqrt(lambda_2) and negated when f_b . (H f_a) < 0 for more rows
 * than > 0.  H with lambda_3 <= 2^-40 lambda_1 is singular.  For exactly four
 * matches, three bearings of one image within 2^-40 of a common plane through
 * the centre (|det(f_i, f_j, f_k)| <= 2^-40: three collinear image points,
 * repeated matches included) leave H undetermined and fail the solve.
 *
 * Decomposition (Ma, Soatto, Kosecka, Sastry, An Invitation to 3-D Vision,
 * 5.3), with lambda_2 = 1: u+- = (sqrt(1 - lambda_3) v_1 +- sqrt(lambda_1 - 1)
 * v_3) / sqrt(lambda_1 - lambda_3), U = [v_2, u, v_2 x u], W = [H v_2, H u,
 * H v_2 x H u], R = W U^T (made a rotation by Gram-Schmidt as above), n = v_2 x
 * u, t / d = (H - R) n: two (R, t / d, n).  For each, the sign of (t, n) is the
 * one for which more rows have n . f_a > 0 (the point is in front of A on the
 * plane), a tie takes the sign as computed, and n_front is that count.  The
 * two are ordered by n_front descending, then by the sum of n . f_a over the
 * rows descending; which of them is the scene's is not decidable from two
 * views.  tau = (lambda_1 - lambda_3) / (sqrt(lambda_1) + sqrt(lambda_3)).
 *
 * The error of (t^, n) grows like eps / tau and calling the motion a rotation
 * costs tau, so at tau <= 2^-24 the call returns count 1: R = H made a
 * rotation, t = 0, the plane 0, n_front = the number of rows.  This guards a
 * 0 / 0; with noise the caller reads tau.
 *
 * A non-finite input, a bearing without direction, a degenerate sample, a
 * singular or non-finite H: every output NaN, count 0, n_front 0.  n = 0 is
 * valid.  NULL buffers (translation excepted) with n > 0:
 * ACM_ERR_INVALID_ARGUMENT.  No workspace, stream-ordered, reentrant.
 *
 * acm_homography_batch: RANSAC over that solver, one 256-lane workgroup per
 * view pair, all pairs in one launch.  The matches (CSR by pair, clamped
 * offsets), the usable-match rule and the bearings (UCM's, FOV's and KB's
 * inverse of the projection, RadTan polished), the records of 48 B in LDS for a pair of at
 * most ACM_HOMOGRAPHY_STAGE_MATCHES matches and in the workspace beyond, and
 * n_usable are acm_relative_pose_batch's.
 *
 * Hypothesis h = 0 .. n_hypotheses - 1 (lanes stride over h) draws local
 * indices with the same splitmix64 and ctr = 8 h + d + 1 for the draws d = 0
 * .. 7.  The first four draws that are usable and pairwise distinct form the
 * sample; otherwise the hypothesis is void.  Its model is the normalised,
 * signed H of the solver above (no decomposition), scored over all usable
 * matches of the pair in order: with g = H f_a and c = f_b x g a match is an
 * inlier iff f_b . g > 0 and c . c <= sin^2(inlier_angle) (g . g) -- f_b lies
 * within inlier_angle of the transferred bearing.  The key of a hypothesis is
 * (inlier count descending, sum over the inliers of c . c / g . g ascending, h
 * ascending), a total order.
 *
 * Refit, as acm_relative_pose_batch's: up to refit_rounds times the rows of
 * the current model's inliers are streamed into R9 (lane l the matches l, l +
 * 256, ...; the fixed butterfly, then the four waves in order), the result
 * normalised, signed by the majority over those inliers and scored; it
 * replaces the model iff strictly better, otherwise the loop ends.  After the
 * last round the final H is decomposed once as above, the cheirality counts
 * and sums taken over the final inliers and added by a fixed tree.
 *
 * Outputs per pair: homography (9 f64, required), status
 * (acm_homography_status, required), n_inliers (required) and, each nullable,
 * poses (two acm_pose), planes (2 x 4 f64), n_solutions (one byte), n_front
 * (two uint32), translation (tau), inlier_mask (one byte per match) and
 * n_usable.  A final H whose decomposition is not finite keeps status OK with
 * n_solutions 0 and NaN motions.  Fewer than 4 usable matches:
 * ACM_HOMOGRAPHY_TOO_FEW_MATCHES.  No hypothesis with a model, or a best count
 * below min_inliers (no refit then): ACM_HOMOGRAPHY_NO_MODEL with n_inliers =
 * the best count (0 without a model).  In both cases n_inliers aside every
 * f64 output is NaN, every count 0 and the pair's mask 0.
 *
 * A pair's outputs depend only on its own match list in order, the camera and
 * the config, and repeated calls return the same bits.  Errors:
 * acm_relative_pose_batch's list with min_inliers < 4 in place of < 8.
 * n_pairs = 0 is valid and touches nothing.  Stream-ordered, no allocation,
 * no host synchronisation, reentrant (two calls in flight need two
 * workspaces).
 *
 * Out of scope: choosing between the essential matrix and the homography;
 * picking one of the two plane solutions (a third view or a known normal
 * does); a non-linear refinement of H; two different cameras per pair. */
ACM_API int acm_homography_4pt(size_t n, const double *bearings_a, const double *bearings_b,
                               double *homography, acm_pose *poses, double *planes,
                               double *translation, uint8_t *count, uint8_t *n_front,
                               void *stream);

typedef enum acm_homography_status {
    ACM_HOMOGRAPHY_OK = 0,
    ACM_HOMOGRAPHY_TOO_FEW_MATCHES = 1, /* fewer than 4 usable matches */
    ACM_HOMOGRAPHY_NO_MODEL = 2         /* no finite model, or fewer than min_inliers inliers */
} acm_homography_status;

/* matches of one pair whose records stay in LDS (48 B each); a longer pair
 * keeps them in the workspace */
#define ACM_HOMOGRAPHY_STAGE_MATCHES 1024

typedef struct acm_homography_config {
    int32_t n_hypotheses;   /* default 256; 1 .. 65536 */
    int32_t flags;          /* must be 0 */
    uint64_t seed;          /* default 1 */
    double inlier_angle;    /* radians, in (0, pi/2); default 5e-3 */
    int32_t min_inliers;    /* default 4; >= 4 */
    int32_t refit_rounds;   /* default 3; 0 .. 8 */
} acm_homography_config;

ACM_API void acm_homography_batch_default_config(acm_homography_config *cfg);
ACM_API size_t acm_homography_batch_workspace_size(size_t n_pairs, size_t n_matches);
ACM_API int acm_homography_batch(const acm_camera *cam, size_t n_pairs,
                                 const int64_t *pair_offsets, size_t n_matches,
                                 const double *uv_a, const double *uv_b,
                                 const acm_homography_config *cfg, double *homography,
                                 uint8_t *status, uint32_t *n_inliers, acm_pose *poses,
                                 double *planes, uint8_t *n_solutions, uint32_t *n_front,
                                 double *translation, uint8_t *inlier_mask, uint32_t *n_usable,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* 3-D similarity alignment (absolute orientation, Horn, Umeyama, Sim(3)): the
 * least-squares b ~ s R a + t between two 3-D point sets, the 3-point solver
 * and RANSAC over it.  It relates two frames that hold the same points: two
 * two-view reconstructions (each in camera A's frame of its pair, in units of
 * its baseline), or a reconstruction and a surveyed frame.  No camera enters
 * these calls: they work on 3-D points alone.
 *
 * A similarity is ACM_SIMILARITY_DOUBLES = 13 f64: R row-major (9), t (3), s.
 *
 * acm_similarity_3pt: n independent problems of three correspondences, one
 * lane each.  points_a, points_b: 9 n f64, problem i holds its three points
 * a_0, a_1, a_2 and b_0, b_1, b_2.  flags: 0, or ACM_SIMILARITY_RIGID for s
 * fixed to 1.  Outputs per problem: similarity (13 f64) and count, one byte, 1
 * or 0.
 *
 * The route, f64 throughout, serves any number n >= 3 of correspondences (the
 * refit below reuses it).  The centroids am, bm; the sums centred on them, M =
 * sum (b - bm)(a - am)^T and Saa = sum |a - am|^2, in index order; Horn's
 * symmetric 4 x 4 matrix N of M (Horn, Closed-form solution of absolute
 * orientation using unit quaternions, 1987), whose largest eigenvalue's
 * eigenvector is the unit quaternion q of R.  The eigenpairs come from a
 * cyclic Jacobi of six sweeps over the six off-diagonal entries, no early
 * exit.  q is signed so that q_0 >= 0 (at q_0 = 0 the first non-zero component
 * is positive) and gives a proper rotation: det R = +1 also for a planar or
 * mirrored set.  s = sum (b - bm) . R (a - am) / Saa = sum_rc R_rc M_rc / Saa
 * (1 with ACM_SIMILARITY_RIGID), t = bm - s R am.  The three points enter
 * through sums only, so the result does not hinge on their order beyond
 * rounding.
 *
 * Void -- every output NaN, count 0: an input or output that is not finite;
 * Saa <= 0 (all a coincide); s <= 0; or, with N's eigenvalues lambda_1 >=
 * lambda_2, not (lambda_1 > 0 and lambda_1 - lambda_2 > 1e-9 lambda_1).  The
 * last covers a collinear configuration (two coincident points included),
 * which leaves the rotation about its line free: its relative gap is at the
 * rounding level, a triangle's well above (>= 2e-4 when sin^2 of the angle at
 * its first vertex is >= 0.01).  n = 0 is valid.  NULL buffers with n > 0 or
 * unknown flag bits: ACM_ERR_INVALID_ARGUMENT.  No workspace, stream-ordered,
 * reentrant.
 *
 * acm_similarity_batch: RANSAC over that solver, one 256-lane workgroup per
 * correspondence set, all sets in one launch.  The correspondences are CSR by
 * set: set k owns the rows set_offsets[k] .. set_offsets[k + 1] - 1 of
 * points_a and points_b (n_points x 3 f64 each); the offsets are clamped into
 * [0, n_points] and a decreasing pair gives an empty set, so nothing is read
 * out of bounds.  A correspondence is usable iff its six values are finite;
 * n_usable (nullable) counts them.  The records, (a, b) of 48 B, stay in LDS
 * for a set of at most ACM_SIMILARITY_STAGE_POINTS correspondences and in the
 * set's own range of six workspace planes beyond.
 *
 * Hypothesis h = 0 .. n_hypotheses - 1 (lanes stride over h) draws local
 * indices with the splitmix64 of acm_pose_estimate_batch and ctr = 6 h + d + 1
 * for the draws d = 0 .. 5.  The first three draws that are usable and
 * pairwise distinct form the sample; otherwise the hypothesis is void, as it
 * is when the solver above is.  The model is scored over all usable
 * correspondences of the set in order: with e = b - (s R a + t) one is an
 * inlier iff e . e <= inlier_distance^2.  The key of a hypothesis is (inlier
 * count descending, sum over the inliers of e . e ascending, h ascending), a
 * total order.
 *
 * Refit: up to refit_rounds times the route above runs over the current
 * model's inliers in two passes -- the centroids, then the centred sums (a
 * one-pass raw-moment form would cancel for sets far from the origin) -- lane
 * l taking the correspondences l, l + 256, ..., the sums added by the fixed
 * butterfly within a wave, then the four waves in order.  The result is
 * scored; it replaces the model iff its key is strictly better, otherwise (or
 * when the fit is void) the loop ends.  A hypothesis' score is added in record
 * order, a refit's score by that fixed tree: at an equal count the comparison
 * is between two summation orders of e . e, so a refit that changes neither
 * the inlier set nor the model beyond rounding is taken or not on the last
 * bits of the two sums -- deterministically, and with the same count and the
 * same score to rounding either way.
 *
 * Outputs per set: similarity (13 f64, required), status
 * (acm_similarity_status, required), n_inliers (required) and, each nullable,
 * rms (sqrt(sum e . e / n_inliers) over the final inliers, added by the same
 * fixed tree), inlier_mask (one byte per correspondence) and n_usable.  Fewer
 * than 3 usable correspondences: ACM_SIMILARITY_TOO_FEW_POINTS.  No hypothesis
 * with a model, or a best count below min_inliers (no refit then):
 * ACM_SIMILARITY_NO_MODEL with n_inliers = the best count (0 without a model).
 * In both cases the similarity and rms are NaN and the set's mask 0.
 *
 * A set's outputs depend only on its own list in order and the config, and
 * repeated calls return the same bits.  Errors (ACM_ERR_INVALID_ARGUMENT,
 * checked even when there is nothing to do): cfg NULL, n_hypotheses outside 1
 * .. 65536, flags other than 0 or ACM_SIMILARITY_RIGID, inlier_distance not
 * finite or <= 0 (the default config holds 0: the caller sets it, in B's
 * units), min_inliers < 3, refit_rounds outside 0 .. 8; with n_sets > 0 a NULL
 * required buffer; a workspace that is NULL or smaller than
 * acm_similarity_batch_workspace_size: ACM_ERR_WORKSPACE_TOO_SMALL.  n_sets =
 * 0 is valid and touches nothing.  Stream-ordered, no allocation, no host
 * synchronisation, reentrant (two calls in flight need two workspaces).
 *
 * Out of scope: weights per correspondence; anisotropic scale; a robust loss
 * in place of the inlier threshold. */
#define ACM_SIMILARITY_DOUBLES 13
/* correspondences of one set whose records stay in LDS (48 B each); a longer
 * set keeps them in the workspace */
#define ACM_SIMILARITY_STAGE_POINTS 1024
#define ACM_SIMILARITY_RIGID 1 /* flags bit 0: s fixed to 1 */

ACM_API int acm_similarity_3pt(size_t n, const double *points_a, const double *points_b,
                               int32_t flags, double *similarity, uint8_t *count, void *stream);

typedef enum acm_similarity_status {
    ACM_SIMILARITY_OK = 0,
    ACM_SIMILARITY_TOO_FEW_POINTS = 1, /* fewer than 3 usable correspondences */
    ACM_SIMILARITY_NO_MODEL = 2        /* no finite model, or fewer than min_inliers inliers */
} acm_similarity_status;

typedef struct acm_similarity_config {
    int32_t n_hypotheses;   /* default 256; 1 .. 65536 */
    int32_t flags;          /* 0 or ACM_SIMILARITY_RIGID */
    uint64_t seed;          /* default 1 */
    double inlier_distance; /* in B's units; finite, > 0; the default config holds 0 */
    int32_t min_inliers;    /* default 3; >= 3 */
    int32_t refit_rounds;   /* default 3; 0 .. 8 */
} acm_similarity_config;

ACM_API void acm_similarity_batch_default_config(acm_similarity_config *cfg);
ACM_API size_t acm_similarity_batch_workspace_size(size_t n_sets, size_t n_points);
ACM_API int acm_similarity_batch(size_t n_sets, const int64_t *set_offsets, size_t n_points,
                                 const double *points_a, const double *points_b,
                                 const acm_similarity_config *cfg, double *similarity,
                                 uint8_t *status, uint32_t *n_inliers, double *rms,
                                 uint8_t *inlier_mask, uint32_t *n_usable, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* Multi-view calibration: the intrinsics and every view's pose in one
 * Levenberg-Marquardt.  K views of known world points, rough poses (device,
 * in/out) and rough intrinsics (cam, host, in/out); the unknowns are the P
 * parameters of the model that are not in fixed_mask, shared by all views,
 * and a 6-DoF pose per view: minimise 0.5 sum ||project_theta(R_k X + t_k) -
 * uv||^2 over theta and the poses.
 *
 * Observations are CSR by view exactly as acm_pose_optimize_batch takes them
 * (view_offsets clamped into [0, n_observations], the same validity rule: a
 * finite pixel, an index in [0, n_points), a finite world point, and an Ok
 * fast projection at the state being evaluated; everything else is skipped,
 * never dereferenced and no error).  A view with fewer than 3 valid
 * observations at the start is ACM_POSE_TOO_FEW_OBSERVATIONS: its pose is
 * left bit for bit, it contributes nothing and is not counted in
 * summary->n_views_used.  No participating view: ACM_LM_FAILED, cam
 * untouched.
 *
 * Per observation the Jacobian row pair is [Jp [I | -[p]x] | Jtheta]: the
 * pose perturbation and retraction are acm_pose_optimize_batch's (left delta
 * = (rho, phi), in double on the device).  The Hessian is an arrow -- K
 * 6 x 6 pose blocks App_k, the P x P block Att and K couplings Atp_k -- and
 * the loop is acm_lm_optimize's state machine on the FULL system, solved
 * through the Schur complement: Marquardt damping A_jj + mu max(A_jj, 1e-12
 * max(dmax, 1)) on every diagonal entry (dmax the largest diagonal entry of
 * the whole system at the first evaluation), L_k = chol(App_k + damping), S =
 * (Att + damping) - sum_k Atp_k App_k^-1 Apt_k and the matching g, summed
 * over the views in view order, dtheta from a Cholesky of S over the free
 * parameters, xn = clamp(x + dtheta), h = xn - x, and per view delta_k =
 * -App_k^-1 (gp_k + Apt_k h).  When the clamp stops a parameter, that
 * parameter is held at its clamped step and S is solved again for the others
 * (the plain projection of a coupled step stalls: DESIGN.md section 8.4);
 * without active bounds nothing changes.  A failed Cholesky in any view block or in S
 * raises mu without an evaluation.  The predicted reduction -(g.h + 0.5 h^T A
 * h) is over the full step with the undamped A; the gain-ratio (Nielsen)
 * update, the three tolerances and the mu > 1e32 failure are
 * acm_lm_optimize's, with the full step's norm against the intrinsics' norm
 * in the parameter test (poses are local: their coordinates are 0).  A trial
 * whose total n_valid is below the current one's is rejected
 * (acm_triangulate's rule).  summary->evaluations counts the evaluations the
 * state machine consumed; a step that ends the run by the parameter
 * tolerance is not among them.
 *
 * Outputs: cam->params and poses receive the best accepted state;
 * max_iterations = 0 leaves both bit for bit and fills every other output at
 * the start.  view_status (device, required): ACM_POSE_TOO_FEW_OBSERVATIONS,
 * or for every participating view ACM_POSE_OK when a tolerance ended the run
 * (or max_iterations = 0) and ACM_POSE_NOT_CONVERGED otherwise.  When
 * non-NULL (device): view_cost (0.5 sum ||r||^2 of the view; NaN for a
 * TOO_FEW view), view_n_valid, and view_system, 256 doubles per view: the
 * 16 x 16 Gram matrix M^T M of the view's augmented Jacobian M = [Jrho Jphi |
 * Jtheta | 0 ... | r] at the returned state -- columns 0-5 the pose, 6 .. 5 +
 * P the intrinsics (every parameter, fixed ones too), column 15 the residual,
 * so [i][15] = (J^T r)_i and [15][15] = r.r; row-major, both triangles,
 * padding exactly 0.  summary (host): information is the undamped reduced S
 * at the returned state, P x P row-major, rows and columns of fixed
 * parameters zero (all zero when a view's undamped pose block is singular).
 *
 * One 256-lane workgroup per view evaluates a state: acm_pose_optimize_batch's
 * staging (views above ACM_POSE_BATCH_STAGE_OBSERVATIONS read global memory
 * at every evaluation, same arithmetic and order), each lane's two rows of M
 * through an LDS tile into v_mfma_f64_16x16x4_f64 rank-4 updates, in a fixed
 * order: repeated calls return the same bits, and inserting a TOO_FEW view
 * anywhere changes no other output bit.  Per iteration: five small launches
 * and two small device-to-host copies, whatever n_views; poses never leave
 * the device.
 *
 * Errors: acm_pose_optimize_batch's list (summary may be NULL), and
 * fixed_mask bits >= P or has_bounds with lower[j] > upper[j] (or a NaN
 * bound): ACM_ERR_INVALID_ARGUMENT.  n_views = 0 is valid and touches
 * nothing.  The call synchronises the stream, as acm_lm_optimize does; no
 * allocation, reentrant. */
typedef struct acm_calibrate_config {
    int32_t max_iterations;      /* default 50; 0 = evaluate only */
    int32_t flags;               /* must be 0 */
    double cost_tolerance;       /* defaults of acm_lm_default_config: 1e-6 */
    double parameter_tolerance;  /* 1e-8 */
    double gradient_tolerance;   /* 1e-6 */
    double initial_damping;      /* 1e-4 */
    uint32_t fixed_mask;         /* bit j set: intrinsic j is held at its start value */
    uint32_t has_bounds;         /* bounds on the intrinsics only, as acm_lm_config */
    double lower[ACM_MAX_PARAMS];
    double upper[ACM_MAX_PARAMS];
} acm_calibrate_config;

typedef struct acm_calibrate_summary {
    int32_t iterations;
    int32_t termination; /* ACM_LM_* */
    int32_t evaluations;
    int32_t n_views_used;
    double initial_cost;
    double final_cost;
    double n_valid;
    double information[ACM_MAX_PARAMS * ACM_MAX_PARAMS];
} acm_calibrate_summary;

ACM_API void acm_calibrate_default_config(acm_calibrate_config *cfg);
ACM_API size_t acm_calibrate_workspace_size(int model, size_t n_views, size_t n_observations);
ACM_API int acm_calibrate(acm_camera *cam, size_t n_views, acm_pose *poses,
                          size_t n_points, const double *points_world,
                          const int64_t *view_offsets, size_t n_observations,
                          const int32_t *obs_point, const double *obs_uv,
                          const acm_calibrate_config *cfg, acm_calibrate_summary *summary,
                          uint8_t *view_status, double *view_cost, uint32_t *view_n_valid,
                          double *view_system, void *workspace, size_t workspace_bytes,
                          void *stream);

/* (r06) The sharded conversion's collectives.  One
 * process per GPU, each holding a shard of the correspondences; both
 * collectives are stream-ordered on device f64 buffers:
 *   allreduce -- in-place sum over the ranks (the acm_allreduce_fn of
 *                acm_lm_optimize / acm_median_valid_allreduce);
 *   allgather -- every rank's `count` values into recv (world x count, in
 *                rank order).
 * acm_rccl_init builds one over an RCCL communicator that libacm drives
 * itself (librccl.so.1: the copy already loaded in the process, e.g.
 * torch's, else ROCm's), so no Python runs per collective; rank 0 makes the
 * id (acm_rccl_unique_id), the caller broadcasts it (e.g. through
 * torch.distributed) and every rank calls acm_rccl_init with its own GPU
 * current -- one GPU per rank.  acm_rccl_destroy frees it.  Any other
 * transport can fill the struct with its own callbacks (the tests' gloo
 * ranks sharing one GPU do). */
typedef int (*acm_allgather_fn)(void *ctx, const double *send, double *recv,
                                size_t count, void *stream);
typedef struct acm_collective {
    acm_allreduce_fn allreduce;
    acm_allgather_fn allgather;
    void *ctx;
    int32_t rank;
    int32_t world;
} acm_collective;
#define ACM_RCCL_UNIQUE_ID_BYTES 128
ACM_API int acm_rccl_available(void);
ACM_API int acm_rccl_unique_id(uint8_t *id);
ACM_API int acm_rccl_init(const uint8_t *id, int32_t world, int32_t rank,
                          acm_collective *out);
ACM_API int acm_rccl_destroy(acm_collective *coll);

/* (r06) convert_to_*'s opening over the union of the ranks' shards
 * (camera_converter.rs:371-375; the multi-GPU form of
 * acm_linear_estimation_with_error_async): per shard the same fused pass
 * (R factor, error flag, the 8 statistics, the median's first histogram),
 * then ONE all-gather of a 32-double record per rank, the rank-ordered
 * Givens merge of the factors and Chan merge of the statistics on the host,
 * the exact median of the union (every histogram summed by coll->allreduce;
 * it lands in initial_error[8] in stream order, initial_error[0..7] hold the
 * union's statistics), and the solve (count checks on the union's size).
 * FOV: the statistics, then the grid sums all-reduced and
 * acm_fov_grid_select.  Every rank gets the same cam->params bit for bit;
 * with one rank (coll NULL, or world 1) the bits of the 1-GPU call.
 * initial_error_host: nullable, host, the union's 8 statistics.
 * cells / grid: nullable, the shard's observations also in the cell form
 * (acm_cell_grid): the fused pass then reads those (same bits); points_2d
 * is still required (the FOV grid search reads pixels). */
ACM_API size_t acm_linear_estimation_with_error_sharded_workspace_size(int model, size_t n,
                                                                       int32_t world);
ACM_API int acm_linear_estimation_with_error_sharded(acm_camera *cam, size_t n,
                                                     const double *points_3d, int layout,
                                                     const double *points_2d,
                                                     const uint32_t *cells,
                                                     const acm_cell_grid *grid,
                                                     double *initial_error,
                                                     double *initial_error_host,
                                                     const acm_collective *coll,
                                                     void *workspace, size_t workspace_bytes,
                                                     void *stream);
/* (r06) compute_reprojection_error (error_metrics.rs:62-121) over the union
 * of the ranks' shards: this shard's statistics pass (with the median's
 * first histogram), one all-gather of the records, Chan's merge, the
 * distributed exact median.  result: device, 9 f64 as acm_reprojection_error
 * (the union's), identical on every rank; errors: nullable device N f64.
 * cells / grid: nullable, the cell form of the observations (then
 * points_2d may be NULL). */
ACM_API size_t acm_reprojection_error_sharded_workspace_size(size_t n, int32_t world);
ACM_API int acm_reprojection_error_sharded(const acm_camera *cam, size_t n,
                                           const double *points_3d, int layout,
                                           const double *points_2d, const uint32_t *cells,
                                           const acm_cell_grid *grid, double *result,
                                           double *errors, const acm_collective *coll,
                                           void *workspace, size_t workspace_bytes,
                                           void *stream);

/* Exact median of the non-NaN values of `values` (the per-point errors of
 * acm_reprojection_stats), error_metrics.rs:103-111: the mean of ranks
 * m/2-1 and m/2 for even m, rank m/2 for odd m, m = n_valid (read from
 * device memory n_valid_device if non-NULL, e.g. result[5] of
 * acm_reprojection_stats, else the host value n_valid).  Values must be
 * >= 0 or NaN.  out: device f64.
 * acm_median_valid_allreduce is the multi-GPU form: `values` is this
 * rank's shard, n_valid the GLOBAL count, and after each of the 6
 * histogram passes the 2 x 2048-bin f64 histogram (device; both median
 * ranks, 11-bit digits) goes through the allreduce callback (a sum over
 * ranks), so every rank selects the same digits and returns the median of
 * the union.  Two passes read all n values; the candidates sharing the
 * selected 22-bit prefix are then compacted into the workspace (which is
 * sized for n of them) and the last four passes read only those. */
ACM_API size_t acm_median_workspace_size(size_t n);
ACM_API int acm_median_valid(size_t n, const double *values,
                             const double *n_valid_device, uint64_t n_valid,
                             double *out, void *workspace,
                             size_t workspace_bytes, void *stream);
ACM_API int acm_median_valid_allreduce(size_t n, const double *values,
                                       const double *n_valid_device,
                                       uint64_t n_valid, double *out,
                                       void *workspace, size_t workspace_bytes,
                                       acm_allreduce_fn allreduce,
                                       void *allreduce_ctx, void *stream);

/* util::sample_points (point_sampling.rs:46-120): a grid of
 * round(sqrt(n*w/h)) x round(sqrt(n*h/w)) cell centres (row-major, as the
 * reference loop), each unprojected; a cell is kept iff the unprojection
 * succeeds and ray.z > 0, in grid order (order-preserving compaction, so
 * indices match the reference's Vec::push order).
 * acm_sample_points_grid (host) gives the grid; the output buffers must hold
 * ncx*ncy points (points_2d_out 2*cap f64, points_3d_out 3*cap f64 AoS).
 * counts (device, 2 x uint64): [kept, ncx*ncy]. */
ACM_API int acm_sample_points_grid(uint32_t width, uint32_t height, size_t n_requested,
                                   uint32_t *num_cells_x, uint32_t *num_cells_y);
ACM_API size_t acm_sample_points_workspace_size(const acm_camera *cam, size_t n_requested);
ACM_API int acm_sample_points(const acm_camera *cam, size_t n_requested,
                              double *points_2d_out, double *points_3d_out,
                              uint64_t *counts, void *workspace,
                              size_t workspace_bytes, void *stream);
/* Same over the cell range [cell_begin, cell_end) of the row-major grid (a
 * multi-GPU shard: ranks take contiguous row ranges and concatenating their
 * outputs in rank order reproduces the serial order).  counts[1] = cells in
 * the range.  Workspace: acm_sample_points_workspace_size of the full grid
 * is always enough. */
ACM_API int acm_sample_points_range(const acm_camera *cam, size_t n_requested,
                                    size_t cell_begin, size_t cell_end,
                                    double *points_2d_out, double *points_3d_out,
                                    uint64_t *counts, void *workspace,
                                    size_t workspace_bytes, void *stream);
/* The host-certified keep regions acm_sample_points counts segments by
 * (inspection / tests; csrc/acm.hip kb_seg_cert): out = [on, all_lo, all_hi,
 * none_lo, none_hi] in the model's certificate variable (KB: ru =
 * min(sqrt(mx^2 + my^2), pi/2); others: r2 = mx^2 + my^2).  Every cell whose
 * variable lies in [all_lo, all_hi] is kept (Ok and z > 0), none in
 * [none_lo, none_hi]; on = 0: no certificate (every segment is counted cell
 * by cell).  Host only. */
ACM_API int acm_sample_points_certificate(const acm_camera *cam, double *out);
/* (r05) RadTan only: the host-certified disk of acm_unproject's fast Newton
 * loop (csrc/acm.hip radtan_newton_disk).  out = [S, fast]: for every (x, y)
 * with x^2 + y^2 <= S the distortion Jacobian has |det| >= 1/16 and
 * |j00| + |j11| + 2 |j01| <= 64, so the loop tests only s <= S per step
 * (S = 0: no disk, the per-step tests); fast = 1 when the certified fast
 * loop runs at all (its distortion bound holds).  Host only; [0, 0] for the
 * other models. */
ACM_API int acm_unproject_certificate(const acm_camera *cam, double *out);
/* (r04) KB only: how acm_sample_points forms the rays of cells inside the
 * certified kept interval.  out = [mode, M, ef, fit_err, all_lo, all_hi]:
 * mode 0 = the reference-iterate path for every cell, 1 / 2 = the root by
 * the fitted initial guess + 1 / 2 Newton steps, 3 = the ray polynomials;
 * M = the Newton error constant, ef = the bound on the distance between the
 * reference's final iterate and the root the certified rays use (modes 1-3
 * require ef <= 1e-11), fit_err = a bound on the ray polynomials' error
 * over the whole certified interval, incl. the device's evaluation rounding
 * (r05: Taylor remainders on 256 pieces, csrc/acm.hip kb_ray_poly_bound;
 * r04 sampled it on 16385 points; mode 3 requires <= 1e-13).  Zeros for
 * other models.  Host only. */
ACM_API int acm_sample_points_ray_fit(const acm_camera *cam, double *out);
/* (r05) KB only: the fitted polynomials themselves, for independent checks
 * of the bounds.  out = 2 * ACM_RAY_POLY_N + ACM_RAY_GUESS_N + 1 doubles:
 * [C_0 .. C_16 | S_0 .. S_16] (cos(theta*) and sin(theta*) / ru in powers of
 * r2; what acm_sample_points evaluates when ray_fit's mode is 3), [g_0 ..
 * g_8] (theta* / ru in powers of r2, the initial guess of modes 1 / 2) and
 * the bound on |ru g(r2) - theta*| over the certified interval.  Zeros when
 * no fit was made.  Host only. */
#define ACM_RAY_POLY_N 17
#define ACM_RAY_GUESS_N 9
ACM_API int acm_sample_points_ray_poly(const acm_camera *cam, double *out);

/* acm_sample_points_range with per-call options: flags = 0 or
 * ACM_REFERENCE_NEWTON.  (acm_sample_points / _range = flags 0.) */
ACM_API int acm_sample_points_ex(const acm_camera *cam, size_t n_requested,
                                 size_t cell_begin, size_t cell_end, int flags,
                                 double *points_2d_out, double *points_3d_out,
                                 uint64_t *counts, void *workspace,
                                 size_t workspace_bytes, void *stream);

/* (r06) acm_sample_points_ex also writing each kept point's grid cell
 * c = i * num_cells_x + j (cells_out: device uint32, cap entries; the
 * grid: acm_sample_points_grid of cam's resolution) -- the cell form of
 * the correspondences for acm_lm_optimize_cells.  Grids of more than
 * 2^32 - 1 cells: ACM_ERR_INVALID_ARGUMENT. */
ACM_API int acm_sample_points_cells(const acm_camera *cam, size_t n_requested,
                                    size_t cell_begin, size_t cell_end, int flags,
                                    double *points_2d_out, double *points_3d_out,
                                    uint32_t *cells_out, uint64_t *counts, void *workspace,
                                    size_t workspace_bytes, void *stream);

/* util::undistort_image (src/util/undistort.rs:14-105).  image/output:
 * device RGB8 row-major, cam->width x cam->height (the reference requires
 * the image to match the model resolution).  target_intrinsics: host
 * [fx fy cx cy] or NULL for the camera's own (:30).  Pixels whose ray fails
 * to project or whose sample falls outside the image are written 0. */
enum { ACM_INTERP_NEAREST = 0, ACM_INTERP_BILINEAR = 1 };
ACM_API int acm_undistort_image(const acm_camera *cam, const double *target_intrinsics,
                                int interpolation, const uint8_t *image,
                                uint8_t *output, void *stream);

/* util::image_quality (src/util/image_quality.rs): the projection rasters
 * of compute_image_quality_metrics, the overlay picture and PSNR / SSIM.
 *
 * A raster is a SET of pixels: every projection is drawn as the 13 pixels
 * with dx^2 + dy^2 <= 4 around (round(u), round(v)) (round half away from
 * zero, then Rust's saturating `as i32`, NaN -> 0; :353-369), clipped to the
 * image, in one colour -- so the result does not depend on the order of the
 * points and a parallel scatter reproduces the reference's sequential loop
 * byte for byte.  Masks are device uint8[height * width], row-major, 1 =
 * drawn.  width and height are 1 .. 2^30.
 *
 * acm_projection_masks (:272-293 + :338-373): one pass over points_3d.  A
 * point is kept iff the input AND the output model project it Ok and the
 * output pixel lies in [0, width) x [0, height) (width / height are the
 * reference image's size when there is one, else the input model's
 * resolution; the cameras' own width / height are not read).  Kept points
 * draw their input pixel into input_mask (not bounds-checked: drawing clips)
 * and their output pixel into output_mask; *n_kept (device uint64) counts
 * them.  Every decision (the filter's bounds test, round()) is that of the
 * reference-exact projections (ACM_EXACT_MATH): by default each lane
 * projects with the default math and only pixels within a guard band of a
 * decision (2e-10 relative, from the default math's 1e-10 bound) are
 * projected again exactly; ACM_RASTER_EXACT_ALL projects every point exactly
 * (the same masks, byte for byte; for measurements).
 * flags: ACM_RASTER_ACCUMULATE ORs into the masks and adds to *n_kept
 * instead of overwriting them (chunks or shards of one point set).  n = 0 is
 * valid: clear masks and a count of 0 (unchanged with the flag).
 * The workspace (acm_projection_masks_workspace_size bytes, 16-B aligned)
 * holds the two bitmasks and the per-workgroup counts.
 *
 * acm_raster_points (create_projection_image, :338-373): the raster of n
 * given pixels (points_2d: 2N f64, interleaved), same workspace size.
 *
 * acm_compose_projection_image (:388-510): per pixel output_rgb where
 * output_mask is set, else input_rgb where input_mask is set, else the
 * background (device RGB8 height x width, NULL = black).  Either mask may be
 * NULL (empty); `image` may be the background buffer itself. */
enum { ACM_RASTER_ACCUMULATE = 1, ACM_RASTER_EXACT_ALL = 2 };
ACM_API size_t acm_projection_masks_workspace_size(uint32_t width, uint32_t height);
ACM_API int acm_projection_masks(const acm_camera *input_cam, const acm_camera *output_cam,
                                 uint32_t width, uint32_t height, size_t n,
                                 const double *points_3d, int layout, int flags,
                                 uint8_t *input_mask, uint8_t *output_mask, uint64_t *n_kept,
                                 void *workspace, size_t workspace_bytes, void *stream);
ACM_API int acm_raster_points(uint32_t width, uint32_t height, size_t n,
                              const double *points_2d, int flags, uint8_t *mask,
                              void *workspace, size_t workspace_bytes, void *stream);
ACM_API int acm_compose_projection_image(uint32_t width, uint32_t height,
                                         const uint8_t *input_mask, const uint8_t *output_mask,
                                         const uint8_t input_rgb[3], const uint8_t output_rgb[3],
                                         const uint8_t *background, uint8_t *image, void *stream);

/* calculate_psnr (:45-89) and calculate_ssim (:108-210) of two device RGB8
 * images (height x width x 3).  result (device, 32 B):
 *   uint64 sse        sum of squared channel differences over the pixel pairs
 *                     that are not black in both images
 *   uint64 valid      3 x the number of those pairs
 *   double ssim_sum   sum of the per-pixel SSIM terms of the interior pixels
 *   uint64 ssim_count number of those terms ((width - 2)(height - 2), or 0)
 * ssim_map (nullable): the (height - 2) x (width - 2) per-pixel terms, each
 * bit-identical to the reference's (no FMA contraction, IEEE divisions).
 * ssim_sum adds per-workgroup partials in index order: the same bits on every
 * run, and within count x 2^-53 of the reference's row-major sum.
 * acm_image_quality_finish (host only): the reference's last steps on a host
 * copy of `result` -- psnr = +inf when valid == 0 or sse / valid <= 1e-10,
 * else 10 log10(255^2 / (sse / valid)) (bit-identical: both sums are exact
 * integers); ssim = ssim_sum / ssim_count, or 1.0 when the count is 0. */
ACM_API size_t acm_image_quality_workspace_size(uint32_t width, uint32_t height);
ACM_API int acm_image_quality(uint32_t width, uint32_t height, const uint8_t *img1,
                              const uint8_t *img2, void *result, double *ssim_map,
                              void *workspace, size_t workspace_bytes, void *stream);
ACM_API int acm_image_quality_finish(const void *result_host, double *psnr, double *ssim);

/* Device-memory helpers so a host without HIP bindings (e.g. the Rust crate
 * through `extern "C"`) can own device buffers: thin wrappers over
 * hipMalloc / hipFree / hipMemcpyAsync / hipStreamSynchronize / hipSetDevice. */
ACM_API int acm_set_device(int device);
ACM_API int acm_device_malloc(void **ptr, size_t bytes);
ACM_API int acm_device_free(void *ptr);
ACM_API int acm_memcpy_htod(void *dst_device, const void *src_host, size_t bytes, void *stream);
ACM_API int acm_memcpy_dtoh(void *dst_host, const void *src_device, size_t bytes, void *stream);
ACM_API int acm_stream_synchronize(void *stream);

/* Process-wide kernel tuning knobs: performance only.  Every knob selects
 * among kernels that return the same results -- bit for bit, except that
 * ACM_TUNE_NE_WAVES / ACM_TUNE_NE_UNROLL / ACM_TUNE_FOV_UNROLL change the
 * summation order of the normal-equations / grid sums (deterministic for a
 * fixed setting, <= ~1e-15 relative apart).  Numerics are never a knob: they
 * are chosen per call (ACM_EXACT_MATH, ACM_REFERENCE_NEWTON).
 * ACM_TUNE_PROJECT_VARIANT: bit flags of acm_project's
 * direct kernel, 1 = non-temporal stores, 2 = persistent grid-stride launch,
 * 4 = non-temporal loads; -1 (default) = auto (non-temporal stores when the
 * outputs exceed 64 MiB; non-temporal loads only if ACM_TUNE_NT_LOADS = 1).  ACM_TUNE_RESIDUAL_NT: non-temporal stores in
 * acm_residual_jacobian (-1 auto, 0 off = default, 1 on).  ACM_TUNE_NE_WAVES:
 * minimum waves per SIMD the normal-equations kernel is compiled for
 * (0 = per-model default, 1, 3, 4).  ACM_TUNE_FOV_UNROLL: the FOV grid search's kernel
 * (-1 = auto (r03) = the point-lane form: lanes own points, every wave
 * walks the grid, sums by wave butterfly -- another summation order, counts
 * identical, sums within ~1e-15; 0 = per-point 64-B records in LDS, each
 * read whole one point ahead (the r03 record form, -1 until r03's point-lane
 * form); 1 / 2 / 4 = the round-2 LDS kernel with 1 / 2 / 4 points per lane
 * step).  acm_fov_grid_workspace_size grew by 2 x 290 doubles (r03).  ACM_TUNE_NE_UNROLL: points per lane step
 * of the normal-equations kernel (0 = per-model default, 1, 2; 3, 4, 5 = one
 * point per step with its loads issued 2, 3, 4 steps ahead; 4 and 5 are
 * Kannala-Brandt only, other models take 3).
 * ACM_TUNE_ALIGN_J: kernel of +Jacobian launches of acm_project /
 * acm_residual_jacobian: -1 = auto (default) = line-aligned store windows
 * through LDS, 0 = one point per lane with direct stores, 1 = aligned.
 * ACM_TUNE_NT_LOADS: non-temporal loads of the point / observation streams
 * in the normal-equations, reprojection-statistics and median kernels
 * (-1 = auto = on, 0, 1; 1 also turns them on in the direct project kernel).  ACM_TUNE_NT_LOADS_UNPROJECT: the same
 * for acm_unproject's pixel stream (-1 = auto = off, 0, 1).
 * ACM_TUNE_LM_HOST_RESULT: acm_lm_optimize without an all-reduce callback
 * has the normal-equations kernel write its results straight into pinned
 * host memory rather than device memory plus a copy: 0 = off, 1 = on with a
 * stream synchronisation, 2 = on with the host spinning on a completion
 * word the kernel publishes, 3 = as 2 with each evaluation queued ahead of
 * the host's decision and released by a host-written doorbell (AoS points,
 * default NE knobs; else 2); -1 = auto = 2.  Every mode takes the same
 * iterates.
 * ACM_TUNE_SAMPLE_FUSED: acm_sample_points' kernels.  -1 = auto (r03) = the
 * speculative segment path (4, below) for RadTan, else the segment two-pass path (certified per-segment counts, offsets by a scan,
 * then a write pass with known offsets); 0 = the round-1 two-pass count /
 * scan / recompute-and-write path (tiles of 16 x 256 cells); 1 / 2 / 3 = the
 * single pass with a decoupled look-back, tiles of 2 / 4 / 8 x 256 cells
 * (round 1 mapped 1 / 2 / 3 to 4 / 8 / 16 x 256; changed in round 2); 4 =
 * speculative segments (r03; auto for RadTan): one pass writes every
 * segment of 64 cells in place as if nothing before it was dropped, a scan
 * gives the true offsets and a repair pass rewrites only the segments after
 * the first drop.
 * Outputs are identical for every value.
 * ACM_TUNE_SAMPLE_CERT: the segment path's host-certified keep regions
 * (-1 = auto = on; 0 = every segment counted cell by cell).  Same outputs.
 * ACM_TUNE_SAMPLE_WRITE: the segment path's write pass, segments per wave
 * and their order (-1 = auto = 16 interleaved across the workgroup's four
 * waves, 4 for KB / UCM / EUCM / FOV; 1 = 64 contiguous, 2 = 16
 * interleaved, 3 = 4 interleaved, 4 = 16 contiguous, 5 = 16 interleaved
 * with non-temporal stores).  Same outputs.
 * ACM_TUNE_UNPROJECT_RCP: unprojections (acm_unproject, acm_sample_points*)
 * divide by fx, fy through the host's correctly rounded 1/fx, 1/fy and one
 * FMA correction, bit-identical to the division (-1 = auto = on, 0 = plain
 * IEEE divisions, 1 = on).
 * ACM_TUNE_SAMPLE_PATIENCE: polls the single-pass sample_points look-back
 * spends on a predecessor tile that has not published its count before the
 * waiting wave counts that tile's cells itself (-1 = auto = 512; 0 = at once,
 * which exercises that path; outputs are identical for every value).
 * ACM_TUNE_NEWTON_FAST (12): removed in round 3 (it changed RadTan's rays by a
 * few ulp process-wide); acm_set_tuning returns ACM_ERR_NOT_SUPPORTED.  Use
 * the per-call ACM_REFERENCE_NEWTON.
 * ACM_TUNE_UNPROJECT_PPT: acm_unproject's pixels per lane and AoS ray
 * stores (-1 = auto = 2 pixels per lane; for Pinhole, DS, UCM and EUCM each
 * wave's 64 AoS rays staged in LDS and written as 16-B pieces when rays is
 * 16-B aligned; 1 / 2 = pixels per lane with three 8-B stores per ray; 3 =
 * 1 pixel per lane, staged when rays is 16-B aligned).
 * Outputs are identical for every value.
 * ACM_TUNE_LM_DEVICE (16): removed in round 5.  Round 4 added it to run the
 * LM state machine on the device behind each evaluation; that loop measured
 * slower than the host loop (1.41 vs 1.33 ms at config 3) and never was the
 * default.  acm_set_tuning returns ACM_ERR_NOT_SUPPORTED; acm_lm_optimize
 * always runs the host loop.
 * ACM_TUNE_ROUND_TRIP (r05): acm_project_unproject's pixels per lane and
 * AoS ray stores: -1 = auto (the per-model default); else PPT (1, 2 or 4)
 * + 8 x stores (0 = the model's default, 1 = each wave's 64 rays staged in
 * LDS and written as 16-B pieces, 2 = three 8-B stores per ray).  Same
 * outputs for every value.
 * Defaults (the value acm_set_tuning returns as "previous" in a fresh
 * process; tests/test_capi.py checks every one): PROJECT_VARIANT -1,
 * RESIDUAL_NT 0, NE_WAVES 0, FOV_UNROLL -1, NE_UNROLL 0, ALIGN_J -1,
 * NT_LOADS -1, NT_LOADS_UNPROJECT -1, LM_HOST_RESULT -1, SAMPLE_FUSED -1,
 * UNPROJECT_RCP -1, SAMPLE_PATIENCE -1, UNPROJECT_PPT -1, SAMPLE_CERT -1,
 * SAMPLE_WRITE -1, ROUND_TRIP -1.
 * Every knob is an atomic: acm_set_tuning may race with any other call.
 * Returns the previous value or an error. */
enum {
    ACM_TUNE_PROJECT_VARIANT = 0,
    ACM_TUNE_RESIDUAL_NT = 1,
    ACM_TUNE_NE_WAVES = 2,
    ACM_TUNE_FOV_UNROLL = 3,
    ACM_TUNE_NE_UNROLL = 4,
    ACM_TUNE_ALIGN_J = 5,
    ACM_TUNE_NT_LOADS = 6,
    ACM_TUNE_NT_LOADS_UNPROJECT = 7,
    ACM_TUNE_LM_HOST_RESULT = 8,
    ACM_TUNE_SAMPLE_FUSED = 9,
    ACM_TUNE_UNPROJECT_RCP = 10,
    ACM_TUNE_SAMPLE_PATIENCE = 11,
    ACM_TUNE_NEWTON_FAST = 12,
    ACM_TUNE_UNPROJECT_PPT = 13,
    ACM_TUNE_SAMPLE_CERT = 14,
    ACM_TUNE_SAMPLE_WRITE = 15,
    ACM_TUNE_LM_DEVICE = 16,
    ACM_TUNE_ROUND_TRIP = 17
};
ACM_API int acm_set_tuning(int key, int value);

/* Diagnostics: last HIP error code / message of the calling thread. */
ACM_API int acm_last_hip_error(void);
ACM_API const char *acm_last_error(void);
ACM_API const char *acm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ACM_H */
