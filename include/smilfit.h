/*
 * libsmilfit - C ABI of the MI355X-native SMIL fitting inner loop.
 *
 * The reference (FabianPlum/SMILify) has no FFI boundary for this path: the path is three
 * Python classes over torch + pytorch3d.  This header is the boundary a binding would use
 * instead; every entry point names the reference code it replaces.  All pointers are DEVICE
 * pointers unless marked "host"; all arrays are dense, row-major fp32 / int32; `stream` is a
 * hipStream_t passed as void*.  Every function returns 0 on success or a negative SMIL_E_*
 * code (message via smil_last_error()); nothing throws, nothing synchronises the device,
 * nothing allocates after smil_model_create() - the caller owns every buffer.
 */
#ifndef SMILFIT_H_
#define SMILFIT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMIL_OK 0
#define SMIL_E_INVALID (-1)  /* bad argument / shape */
#define SMIL_E_DEVICE (-2)   /* HIP runtime error */
#define SMIL_E_UNSUPPORTED (-3)

#define SMIL_MAX_BONES 4     /* bones per vertex in the skin table */
#define SMIL_MAX_JOINTS 256
#define SMIL_MAX_BETAS 64
#define SMIL_MAX_FACES_PER_PIXEL 128

typedef struct SmilModel SmilModel; /* opaque: device-resident model constants */

/* Host-side description of a model.  Replaces the buffers built in SMAL.__init__
 * (reference smal_model/smal_torch.py:104-196).  All pointers are HOST pointers. */
typedef struct {
    int32_t V, F, J, nB;
    const float *v_template;    /* (V,3) */
    const float *shapedirs;     /* (nB,3V), inner index v*3+c */
    const int32_t *faces;       /* (F,3) */
    const int32_t *parents;     /* (J,), parents[0] = -1, parents[i] < i */
    const int32_t *skin_idx;    /* (V,4) bone ids (padding: id 0, weight 0) */
    const float *skin_w;        /* (V,4) */
    const int32_t *jreg_rowptr; /* (J+1,) joint regressor, CSR by joint */
    const int32_t *jreg_col;    /* (nnz,) vertex ids */
    const float *jreg_val;      /* (nnz,) */
    int32_t static_joints;      /* config.STATIC_JOINT_LOCATIONS (smal_torch.py:175,257,343) */
    const float *J_static;      /* (J,3) when static_joints */
    const float *posedirs;      /* (9(J-1),3V) pose blend shapes (smal_torch.py:178-190) or NULL when empty / all zero */
} SmilModelDesc;

int smil_model_create(const SmilModelDesc *desc, SmilModel **out);
void smil_model_destroy(SmilModel *m);
int smil_model_dims(const SmilModel *m, int32_t dims[4]); /* V,F,J,nB */
const char *smil_last_error(void);
const char *smil_version(void);   /* "smilfit 0.13 (gfx950; 0.3 + SmilCameras.principal (0.4) + fragments, depth visibility (0.5) + mesh-free joints, kp3d fit (0.6) + kp2d fit (0.7) + visual hull (0.8) + distance fields (0.9) + hull meshes (0.10) + point-mesh distances (0.11) + winding numbers (0.12) + mesh BVH)".  0.13 adds
                                    * the smil_bvh_* entry points and changes no layout.  0.12 adds
                                    * smil_point_mesh_winding and changes no layout.  0.11 adds
                                    * smil_point_face_distance / smil_face_point_distance / smil_point_mesh_backward and their
                                    * workspace query and changes no layout.  0.10 adds
                                    * the smil_hull_mesh_* entry points and changes no layout.  0.9 adds
                                    * smil_hull_edt, its workspace query and smil_field_sample and changes no layout.  0.8 adds
                                    * the smil_hull_* entry points with their own struct and changes no layout.  0.7 adds
                                    * smil_kp2d_fit_eval and its workspace query and changes no layout.  0.6 adds
                                    * smil_joints_forward / smil_joints_backward / smil_kp3d_fit_eval / smil_adam_step_multi_bc64 with their own structs and changes no layout.
                                    * 0.3 = the layout of rounds 5 - 6: SmilLbsGrads carries clip_depth in front of
                                    * beta_rows (which must hold 2 * B * nB_used + 16 floats), SmilRasterSettings ends in {tie_rule, clip_depth,
                                    * image0}, smil_window_terms exists.  0.4: SmilCameras ends in {principal, nPrincipal} (a zero-initialised
                                    * struct means what it meant in 0.3).  0.5 adds smil_render_fragments and
                                    * smil_depth_visibility and changes no layout.  Callers zero-initialise every struct they pass and rebuild against
                                    * this header when the number changes: there is no binary compatibility across it. */

/* ------------------------------------------------------------------------------------------
 * Linear blend skinning.  Replaces SMAL.__call__ (smal_torch.py:198-370) including
 * batch_rodrigues (batch_lbs.py:31-50) and batch_global_rigid_transformation (batch_lbs.py:75-197).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t B;
    int32_t shared_beta;        /* 1: beta is one (nB_used,) row used by every frame */
    int32_t nB_used;            /* beta.shape[1] in the reference call (<= nB) */
    const float *beta;          /* (B,nB_used) or (nB_used,) */
    const float *theta;         /* (B,J,3) axis-angle, or NULL when Rs_in is given */
    const float *Rs_in;         /* (B,J,3,3) rotation matrices passed directly (smal_torch.py:288) */
    const float *logscale;      /* betas_logscale (B,J,3) / (J,3) / NULL */
    int32_t logscale_shared;    /* 1: one (J,3) table for every frame */
    const float *btrans;        /* betas_trans, same conventions */
    int32_t btrans_shared;
    const float *trans;         /* (B,3) or NULL */
    int32_t trans_after_joints; /* 0: SMAL.__call__ semantics - joints are regressed from the translated
                                   vertices (smal_torch.py:340-351); 1: SMALFitter semantics - trans is added
                                   to verts AND joints after regression (fitter.py:280-281) */
    const float *del_v;         /* (B,V,3) or NULL */
    const float *v_template;    /* (V,3) override or NULL */
    int32_t propagate_scaling;  /* batch_lbs.py:163-168 */
    int32_t allow_limb_scaling; /* config.ALLOW_LIMB_SCALING (batch_lbs.py:123) */
    const float *theta_mask;    /* (J,3) or NULL: theta is used as theta * mask (global_mask / rotation_mask of
                                   SMALFitter.forward, fitter.py:242-243) without a masked copy; d_theta is the gradient
                                   with respect to the MASKED pose */
} SmilLbsInputs;

typedef struct {
    float *v_shaped; /* (nS,V,3); nS = 1 when shared_beta && !del_v, else B */
    float *J_rest;   /* (nS,J,3) rest joints */
    float *Rs;       /* (B,J,3,3) */
    float *G;        /* (B,J,3,4) world transforms, saved for backward */
    float *A;        /* (B,J,3,4) relative skinning transforms */
    float *new_J;    /* (B,J,3) = SMAL.J_transformed */
    float *verts;    /* (B,V,3) */
    float *joints;   /* (B,J,3) */
    float *v_posed;  /* (B,V,3) v_shaped + pose blend shapes; required iff the model has posedirs, else NULL */
} SmilLbsOutputs;

int smil_lbs_forward(const SmilModel *m, const SmilLbsInputs *in, const SmilLbsOutputs *out, void *stream);

/* Depth gradients of the end points of edges that cross the rasteriser's clipping plane (pytorch3d clip_faces differentiates the
 * crossing point through w = (z_a - z_clip) / (z_a - z_b) and the explicit depth factors; the reference leaves clipping on,
 * p3d_renderer.py:36-47).  A sparse side channel next to d_ndc (N,V,2): the silhouette backward entry points append, per image that
 * has cut faces, entries {vertex, d loss / d z_view[vertex]} and record the image's run in `range`; smil_lbs_backward_ndc and
 * smil_clip_depth_backward carry them through the camera (z_view = X_world . R[:,2] + T_z) into the world-space vertex gradient.
 * All buffers are the caller's.  No BASELINE configuration cuts a face: the channel stays empty there and costs one word read. */
typedef struct {
    int32_t *vertex;      /* (capacity) */
    float *dz;            /* (capacity) */
    uint32_t *range;      /* (N_total, 2): first entry and number of entries of every image of the caller's batch */
    uint32_t *counter;    /* [0] entries in use (reset by the call whose image0 == 0), [1] entries that did not fit (dropped, counted) */
    int32_t capacity;
} SmilClipDepth;

typedef struct {
    const float *d_verts;  /* (B,V,3) upstream gradient or NULL */
    const float *d_joints; /* (B,J,3) upstream gradient or NULL */
    float *d_beta;         /* (B,nB_used) or (nB_used,); NULL to skip */
    float *d_theta;        /* (B,J,3); NULL to skip (ignored when Rs_in was used) */
    float *d_logscale;     /* (B,J,3) or (J,3) when shared; NULL to skip */
    float *d_btrans;       /* same */
    float *d_trans;        /* (B,3); NULL to skip */
    /* scratch owned by the caller */
    float *d_A;            /* (B,J,3,4) */
    float *d_Jrest;        /* (B,J,3) */
    float *d_Rs;           /* (B,J,3,3) */
    float *d_vposed;       /* (B,V,3): required iff the model has posedirs */
    float *d_posefeat;     /* (B,9(J-1)): required iff the model has posedirs */
    float *d_del_v;        /* (B,V,3) or NULL: gradient on the per-frame vertex offsets del_v (smal_torch.py:244-248);
                              also the gradient on v_shaped / v_template rows of each frame */
    float *d_Rs_in;        /* (B,J,3,3) or NULL: gradient on the rotation matrices when theta was given as
                              matrices (Rs_in; smal_torch.py:288-289) */
    int32_t accumulate_shared_beta; /* shared_beta only: ADD the sum over frames to d_beta (caller zeroes it or holds
                              other terms there) instead of overwriting it */
    const float *up_Rs;       /* (B,J,3,3) or NULL: upstream gradient on the rotation matrices the forward returned
                              (SMAL.__call__ hands Rs to its caller, smal_torch.py:367-370); flows to d_theta / d_Rs_in */
    const float *up_v_shaped; /* (nS,V,3) or NULL: upstream gradient on the returned v_shaped; flows to d_beta and d_del_v */
    const SmilClipDepth *clip_depth; /* or NULL (smil_lbs_backward_ndc only): depth gradients from the rasteriser's clipping plane,
                              added to the frame's vertex gradient through the cameras */
    float *beta_rows;         /* scratch, 2 * B * nB_used + 16 floats: required iff shared_beta and d_beta.  The kernels leave one partial
                              sum per block there and the last block to finish adds them in a fixed order; the word behind the rows
                              counts the finished blocks of THIS call (cleared by the call's own kernels: calls with different
                              scratch may run on different streams) */
} SmilLbsGrads;            /* every output is overwritten; tables shared by all frames (shared_beta,
                              logscale_shared, btrans_shared) receive the sum over frames.  All of these sums are taken in a
                              fixed order: two calls on the same inputs return the same bits (the shared shape gradient - the
                              quantity ranks all-reduce - included, since round 4) */

int smil_lbs_backward(const SmilModel *m, const SmilLbsInputs *in, const SmilLbsOutputs *saved,
                      const SmilLbsGrads *g, void *stream);

/* ------------------------------------------------------------------------------------------
 * Cameras + projection.  Replaces FoVPerspectiveCameras as configured by Renderer
 * (p3d_renderer.py:34-38,112-120) and transform_points_screen(...)[..., [1,0]] (:137).
 * Image n = frame * views + view.  A table with k rows is indexed n % k (k = 1, views or N).
 * With `principal` the cameras are pytorch3d's PerspectiveCameras (NDC) instead: the same R, T, K00 = 1 / (aspect tan(fov/2)),
 * K11 = 1 / tan(fov/2) and a principal point added to x_ndc, y_ndc - what a calibrated pinhole (cx, cy off centre) or a crop
 * window of a larger frame needs.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t N;          /* images = frames * views */
    int32_t views;      /* views per frame (>= 1) */
    int32_t S;          /* square image side */
    const float *R;     /* (nR,3,3) row-vector convention: X_view = X_world R + T */
    int32_t nR;
    const float *T;     /* (nT,3) */
    int32_t nT;
    const float *fov;   /* (nFov,) degrees */
    int32_t nFov;
    const float *aspect; /* (nAspect,) or NULL = 1 */
    int32_t nAspect;
    const float *principal; /* (nPrincipal,2) principal point (px, py) in NDC, or NULL = centred (0, 0): pytorch3d's PerspectiveCameras,
                               x_ndc = K00 x_view / z_view + px, y_ndc = K11 y_view / z_view + py; the screen transform is unchanged
                               (x_s = S/2 - (S/2) x_ndc).  Under the OpenCV conversion R = R_cv^T diag(-1,-1,1) a pinhole u = fx x/z + cx
                               on an S x S image has px = 1 - 2 cx / S, py = 1 - 2 cy / S.  Values outside [-1, 1] are valid (a crop
                               window whose principal point lies outside it).  A constant of the fit: no entry point returns a
                               gradient on it, and the backward entry points' results do not depend on it. */
    int32_t nPrincipal;     /* > 0 when principal is given */
} SmilCameras;

/* pts (frames,P,3) world -> ndc (N,P,3) = (x_ndc, y_ndc, z_view); yx (N,P,2) = (y_s, x_s) px. Either
 * output may be NULL. */
int smil_project(const SmilCameras *cam, const float *pts, int32_t P, float *ndc, float *yx, void *stream);

/* Two point sets through the same cameras in one launch (the vertices for the rasteriser and the joints for the 2-D
 * loss of one fit iteration); arguments per set as smil_project. */
int smil_project2(const SmilCameras *cam, const float *pts_a, int32_t Pa, float *ndc_a, float *yx_a, const float *pts_b,
                  int32_t Pb, float *ndc_b, float *yx_b, void *stream);

/* smil_project_backward for two point sets in one launch (d_pts of both overwritten; d_fov_img added to).  d_ndc_scale_a:
 * as in smil_project_backward, for set a. */
int smil_project_backward2(const SmilCameras *cam, const float *pts_a, int32_t Pa, const float *d_ndc_a, const float *d_yx_a,
                           float *d_pts_a, const float *pts_b, int32_t Pb, const float *d_ndc_b, const float *d_yx_b,
                           float *d_pts_b, float *d_fov_img, const float *d_ndc_scale_a, void *stream);

/* Backward of smil_project.  d_ndc (N,P,2) and/or d_yx (N,P,2) -> d_pts (frames,P,3) (summed over
 * views; overwritten unless accumulate) and d_fov_img (N,): per-image raw sums
 * sum_p (d x_ndc * x_ndc + d y_ndc * y_ndc), ATOMICALLY ADDED (caller zeroes once, then may call this for
 * several point sets).  smil_fov_reduce turns them into d_fov (nFov,), overwritten.
 * d_ndc_scale (N,) or NULL: the per-image decode factors smil_silhouette_l1_fused returned with a d_ndc it left packed
 * (> 0: the row is 64-bit packed fixed point, times this factor; 0: plain floats; < 0: a packed row of zeros). */
int smil_project_backward(const SmilCameras *cam, const float *pts, int32_t P, const float *d_ndc,
                          const float *d_yx, float *d_pts, float *d_fov_img, int32_t accumulate, const float *d_ndc_scale,
                          void *stream);
int smil_fov_reduce(const SmilCameras *cam, const float *d_fov_img, float *d_fov, void *stream);

/* smil_lbs_forward followed by the projection of its vertices and joints through `cam` (N = in->B * cam->views images):
 * ndc (N,V,3) as smil_project(verts) and yx (N,J,2) as smil_project(joints); either may be NULL.  Replaces SMAL.__call__
 * + Renderer's two projections of one fit iteration (fitter.py:270-290, p3d_renderer.py:137-146).  Skinning, joint regression and
 * both projections are ONE kernel per frame and `verts` is written once and not read back where the model's joints are static
 * (nothing is gathered from the frame's vertices: any mesh size) or the frame's vertices fit half a CU's LDS (3 V floats <= 80 KB);
 * otherwise the separate kernels run.  Outputs are those of the separate calls: to rounding (1e-6 of the largest entry) through the
 * fused kernel, and BIT FOR BIT where the separate kernels run - which they always do for cameras with a principal point: with a
 * table this call is specified to return exactly what smil_lbs_forward followed by smil_project returns. */
int smil_lbs_forward_project(const SmilModel *m, const SmilLbsInputs *in, const SmilLbsOutputs *out, const SmilCameras *cam,
                             float *ndc, float *yx, void *stream);

/* smil_lbs_backward taking its upstream gradients on the IMAGE PLANE, as the fit iteration has them: d_ndc (N,V,2) on the
 * projected vertices (rows may be the packed fixed point smil_silhouette_l1_fused leaves, with d_ndc_scale (N,) as in
 * smil_project_backward) and d_yx_joints (N,J,2) on the projected joints (y, x) in pixels; either may be NULL.  One kernel per
 * frame does what smil_project_backward2 + smil_lbs_backward do (backward of p3d_renderer.py:137-146 into the backward of
 * smal_torch.py:240-351) without writing the (B,V,3) vertex gradient to memory.  g->d_verts, g->d_joints and g->d_del_v
 * must be NULL; d_joints (B,J,3) receives the world-space joint gradient (an output); d_fov_img (N,) or NULL is ADDED to
 * as by smil_project_backward.  saved->verts and saved->joints are read.  Results equal the two-call route up to fp32
 * summation order.  smil_lbs_backward_ndc_supported: 1 when this entry handles the model with nB_used shape coefficients (<= 9)
 * and `views` views per frame (<= 32): no pose blend shapes, and either the frame's vertex gradient AND rest vertices fit half a
 * CU's LDS (24 V bytes <= 80 KB: two workgroups of 512 threads per CU) or the vertex gradient alone fits the CU's whole LDS
 * (12 V bytes <= 160 KB, V <= ~13 000: one workgroup of 1024 threads per CU, rest vertices gathered from memory). */
int smil_lbs_backward_ndc(const SmilModel *m, const SmilLbsInputs *in, const SmilLbsOutputs *saved, const SmilLbsGrads *g,
                          const SmilCameras *cam, const float *d_ndc, const float *d_ndc_scale, const float *d_yx_joints,
                          float *d_joints, float *d_fov_img, void *stream);
int smil_lbs_backward_ndc_supported(const SmilModel *m, int32_t nB_used, int32_t views);
/* The separate-kernel route's counterpart of SmilLbsGrads.clip_depth: d_verts (B,V,3) += the depth gradients of `cd` carried through
 * the cameras (image n belongs to frame n / views).  Call after smil_project_backward{,2}. */
int smil_clip_depth_backward(const SmilCameras *cam, const SmilClipDepth *cd, int32_t N, int32_t V, float *d_verts, void *stream);

/* ------------------------------------------------------------------------------------------
 * Soft silhouette.  Replaces MeshRasterizer(naive, K faces per pixel, blur) + SoftSilhouetteShader
 * (p3d_renderer.py:41-52,142-146; arithmetic in un-vendored pytorch3d 0.7.8).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    float blur_radius;        /* NDC^2; reference: log(1/1e-4 - 1) * 1e-4 */
    float sigma;              /* 1e-4 */
    int32_t faces_per_pixel;  /* K = 100 */
    float z_clip;             /* MeshRasterizer's z_clip_value = znear / 2 = 5e-4: faces whose three vertices are all
                                 nearer than this are culled, faces that cross it are cut there (clip_faces) */
    int32_t tie_rule;         /* which faces a pixel keeps among EQUAL depths at its K-th place.  SMIL_TIE_DEPTH_FACE_ID (0, default):
                                 the smallest face ids - order independent, what the tile kernel computes.  SMIL_TIE_REFERENCE_QUEUE (1):
                                 what pytorch3d's unsorted K-queue ends up with when it visits the faces in index order (the
                                 reference's rasteriser, p3d_renderer.py:42-47): such pixels (~2 % of the truncated ones) are replayed
                                 one by one by a second kernel.  Measured difference on the L1 term: ~1e-5 relative at K = 100 */
    const SmilClipDepth *clip_depth; /* or NULL: where smil_silhouette_backward / smil_silhouette_l1_fused leave the depth gradients of
                                 cut edges' end points (NULL: dropped - the xy gradients are complete either way) */
    int32_t image0;           /* index of this call's first image in the caller's batch (`clip_depth->range` is indexed by it): a
                                 batch cut into several calls passes 0, N_1, N_1 + N_2, ... */
} SmilRasterSettings;
#define SMIL_TIE_DEPTH_FACE_ID 0
#define SMIL_TIE_REFERENCE_QUEUE 1

/* Caller-owned scratch for N images of side S: per-face tile boxes / depth ranges, the tile work list, and the pair-record
 * streams of the resident workgroups (about 1.6 MB each, 16 per CU: 6.6 GB once N * tiles exceeds that many - size the
 * buffer once and reuse it).  Meshes with more than 65536 faces are rejected (SMIL_E_INVALID). */
size_t smil_raster_workspace_bytes(const SmilModel *m, int32_t N, int32_t S);

/* Counters of the most recent rasteriser call that used `workspace`, whatever its N, copied to out4[4] (synchronises the
 * stream): [0] faces that cross z_clip (one or two vertices nearer than znear / 2): cut at the plane like pytorch3d's
 * clip_faces, which p3d_renderer.py:36-47 leaves on - the front part is rendered as one or two extra triangles whose new
 * vertices hand their gradient back to the cut edge's end points: to their xy through d_ndc, to their DEPTHS - the crossing
 * point also moves with z_a and z_b - through SmilRasterSettings.clip_depth (a sparse list; dropped when NULL).  [1] touched 8x8 tiles.  [2] faces that cross the plane beyond the capacity of the per-image clip tables - 1024 cut faces per
 * image, each with up to two front-part triangles and two new vertices: rendered whole, or not at all when a vertex is nearer than 1e-8 - the one case in which a call still deviates.
 * [3] pixels whose tie group at the K-th depth was cut by K and that were therefore replayed through the reference's queue
 * (tie_rule = SMIL_TIE_REFERENCE_QUEUE only; 0 otherwise). */
int smil_raster_stats(const SmilModel *m, const void *workspace, void *stream, uint32_t *out4);

/* verts_ndc (N,V,3) -> sil (N,S,S) */
int smil_silhouette_forward(const SmilModel *m, const float *verts_ndc, int32_t N, int32_t S,
                            const SmilRasterSettings *rs, float *sil, void *workspace, void *stream);
/* grad_sil (N,S,S) -> d_ndc (N,V,2) (overwritten) */
int smil_silhouette_backward(const SmilModel *m, const float *verts_ndc, int32_t N, int32_t S,
                             const SmilRasterSettings *rs, const float *grad_sil, float *d_ndc,
                             void *workspace, void *stream);
/* Fused forward + L1 against a target + backward, no silhouette materialised (SMALFitter path,
 * fitter.py:332-333): loss_img[n] = sum_px |sil - target|, d_ndc (N,V,2) = d(sum_n pix_scale[n] *
 * loss_img[n]) / d ndc.  target_sum[n] = sum_px target (constant, computed once by the caller) lets
 * untouched tiles skip their target read.  target is (N,S,S) fp32, or uint8 holding binary {0,1} masks when
 * target_is_u8 (a quarter of the memory and read traffic).  sil_out may be NULL.  loss_img is bit-reproducible: the tiles'
 * terms are summed as 2^-32 fixed-point integers (any order of arrival) and added to target_sum[n] once.
 * From 64 images per call on (and an 8-byte aligned d_ndc), d_ndc is accumulated as 64-bit packed fixed point in the same
 * buffer: every (face, pixel) contribution is rounded once to 2^-30 of a per-image worst-case bound (vertex valence x largest
 * face pixel box x 0.4 |pix_scale| / sqrt(sigma)) and all further sums are integer adds - independent of the order in which
 * tiles finish and of how faces are grouped (bit-reproducible).  Relative to an image's largest gradient component that is
 * ~2e-6 on ordinary meshes and up to a few 1e-4 when one face fills the image (the bound grows with the largest face box);
 * smaller calls, and images with faces cut at z_clip, use float atomics (order-dependent last bits).
 * d_ndc_scale == NULL: packed rows are decoded in place before the call's work ends on the stream - the caller always sees
 * floats.  d_ndc_scale (N,) given: no decode pass; d_ndc_scale[n] says how image n's row is to be read (see
 * smil_project_backward, which takes the pair as it is and decodes while it reads). */
int smil_silhouette_l1_fused(const SmilModel *m, const float *verts_ndc, int32_t N, int32_t S,
                             const SmilRasterSettings *rs, const void *target, int32_t target_is_u8,
                             const float *target_sum, const float *pix_scale, float *loss_img, float *d_ndc,
                             float *sil_out, float *d_ndc_scale, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * Colour (HardPhong) rendering.  Replaces the reference Renderer's colour branch (p3d_renderer.py:54-70,148-150: MeshRasterizer with
 * blur_radius 0, faces_per_pixel 1, bin_size 0 on the same cameras + HardPhongShader with PointLights(location [[0, 0, 3]]), default
 * Materials / BlendParams, TexturesVertex of one colour), used by render_texture=True (p3d_renderer.py:127-150) and by
 * SMALFitter.generate_visualization (fitter.py:462-480).  Lights and materials are the reference's constants; the mesh colour is the
 * only input.  No gradient.
 * ---------------------------------------------------------------------------------------- */
/* Caller-owned scratch for N images of side S (per-face tile boxes / depth ranges, binned tile lists, work items, clip tables of the
 * faces cut at z_clip, vertex normals): about 12 F + 8 x LIST entries of 8 B per image - no per-workgroup pair-record streams. */
size_t smil_colour_workspace_bytes(const SmilModel *m, int32_t N, int32_t S);
/* verts_world (frames,V,3) world-space vertices, verts_ndc (N,V,3) = smil_project(cam, verts_world) (N = cam->N = frames * views,
 * S = cam->S), rgb[3] a HOST array (MESH_COLOR / 255) -> image (N,3,S,S) planar RGB, background (1,1,1); pix_to_face (N,S,S) the
 * original face id of every pixel (-1: background) or NULL.  z_clip = znear / 2 as on the silhouette path; faces cut there are drawn
 * as pytorch3d's clip_faces cuts them and reported as their original face.  A pixel shows the smallest (depth, face, part). */
int smil_render_colour(const SmilModel *m, const SmilCameras *cam, const float *verts_world, const float *verts_ndc,
                       const float rgb[3], float *image, int32_t *pix_to_face, void *workspace, void *stream);
/* ------------------------------------------------------------------------------------------
 * Fragments of the hard rasteriser, and keypoint self-occlusion against a depth buffer.  smil_render_fragments hands out what
 * pytorch3d's MeshRasterizer (blur_radius 0, faces_per_pixel 1, bin_size 0: p3d_renderer.py:54-70) returns as Fragments and the colour
 * path uses for one pixel of shading; smil_depth_visibility replaces Unreal2Pytorch3D.py:664-760 (refine_visibility_with_depth, called
 * per view at :1558-1580) for all images of a batch.  No gradient.
 * ---------------------------------------------------------------------------------------- */
/* Caller-owned scratch for N images of side S: the tables of the colour path's setup alone (no vertex normals). */
size_t smil_fragments_workspace_bytes(const SmilModel *m, int32_t N, int32_t S);
/* The rasterisation of smil_render_colour (same arguments, same rule: a pixel shows the smallest (depth, face, part)) without the
 * shading.  Every output may be NULL (at least one is not):
 *   pix_to_face (N,S,S)    original per-mesh face id, -1 for background
 *   zbuf        (N,S,S)    view depth of the winner, -1 for background
 *   bary        (N,S,S,3)  perspective-correct, unclipped barycentrics with respect to the original face, -1 for background
 *   dist        (N,S,S)    |C - X|: Euclidean distance from the camera centre C = -T R^T to the world point X = sum_c b_c
 *                          verts_world[P_c], formed as the colour path forms them; +inf for background
 * There is no K axis and no `dists` (K = 1, blur 0).  verts_world (frames,V,3) and the camera tables R, T are read only for dist and
 * may be NULL without it.  Two calls give the same bits. */
int smil_render_fragments(const SmilModel *m, const SmilCameras *cam, const float *verts_world, const float *verts_ndc,
                          int32_t *pix_to_face, float *zbuf, float *bary, float *dist, void *workspace, void *stream);
/* Unreal2Pytorch3D.py:733-758 for B images of P keypoints each, every comparison in float64.  depth: with depth_is_u8 a (B,H,W,channels)
 * uint8 buffer whose channel 0 encodes surface = (r / 255.0) * depth_max (the minimum over the window is taken on the bytes); otherwise
 * (B,H,W) float32 distances, +inf for background (channels and depth_max are ignored).  kp_norm (B,P,2) float64 = (norm_x, norm_y) with
 * norm_x along the ROWS (the reference's swapped convention): row = min(max(trunc(norm_x H), 0), H - 1), col likewise from norm_y W.
 * kp_dist (B,P) float64 the keypoint's distance to the camera (non-finite: no 3-D position).  neighborhood = half-window h in [0, 8]
 * (otherwise SMIL_E_INVALID): rows [max(0, row - h), min(H, row + h + 1)), columns likewise.
 * vis_out (B,P) = vis_in, except 0 where vis_in != 0, kp_dist is finite, 0 <= norm_x, norm_y <= 1 (a NaN fails) and
 * kp_dist > surface + tolerance.  surface (B,P) float64 or NULL: the sampled minimum, NaN where no sample was taken.  vis_out may be
 * vis_in. */
int smil_depth_visibility(const void *depth, int32_t depth_is_u8, int32_t channels, double depth_max, int32_t B, int32_t H, int32_t W,
                          const double *kp_norm, const double *kp_dist, int32_t P, const float *vis_in, double tolerance,
                          int32_t neighborhood, float *vis_out, double *surface, void *stream);
/* Measurement hook (bench.py): when enabled, every launch of the tile kernel is bracketed by HIP events on its
 * launch stream; smil_profile_read synchronises those events and returns their summed duration + count. */
int smil_profile_enable(int32_t on);
int smil_profile_read(float *total_ms, int32_t *launches);

/* ------------------------------------------------------------------------------------------
 * Priors / joint loss / temporal / Adam.  Replaces the loss block of SMALFitter.forward
 * (fitter.py:292-333), get_temporal (:337-350) and the Adam step of optimize_to_joints.py:117-175.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int32_t N;            /* frames held by this rank */
    int32_t J;            /* joints incl. root */
    int32_t nB;
    int32_t window;       /* config.WINDOW_SIZE: losses are means per window, summed over windows */
    int32_t frame0;       /* global index of local frame 0 (multi-GPU shard offset) */
    int32_t N_total;      /* frames of the whole sequence */
    float w_j2d, w_reproj, w_betas, w_pose, w_limit, w_splay, w_temp;
    float limit;          /* joint limit half-width (0.01) */
    int32_t train_global, train_joints, train_trans; /* requires_grad of the per-frame groups
                                                        (optimize_to_joints.py:129-144): 0 -> gradient zeroed */
} SmilFitConfig;

/* objs is a 10-float accumulator, every entry ADDED to (caller zeroes once per iteration):
 * [0] joint  [1] limit  [2] pose  [3] splay  [4] betas  [5] sil_reproj
 * [6] temporal joint-rotations  [7] temporal global-rotation  [8] temporal translation  [9] unused */
#define SMIL_N_OBJS 10

/* Prior terms (limit, pose, splay, betas, temporal) and their gradients on the per-frame parameters.
 * pose (N,J,3): row 0 of each frame = global_rotation, rows 1.. = joint_rotations (UNMASKED parameters);
 * mask (J,3): row 0 = global_mask, rows 1.. = rotation_mask (fitter.py:213-219,242-243); trans (N,3);
 * betas (nB,).  halo_prev / halo_next: the (3J+3,) row [pose, trans] of the frame just before / after this
 * shard (NULL at the sequence ends).
 * accumulate = 1: d_pose holds gradients w.r.t. the MASKED pose on entry (from smil_lbs_backward) and the
 * final parameter gradients on exit ((in + prior) * mask * train flag); d_trans is added to.
 * accumulate = 0: overwritten.  d_betas (nB,) is ADDED to. */
int smil_prior_losses(const SmilFitConfig *cfg, const float *pose, const float *trans, const float *betas,
                      const float *mean_betas, const float *betas_prec, const float *mask,
                      const float *halo_prev, const float *halo_next, float *objs, float *d_pose,
                      float *d_trans, float *d_betas, int32_t accumulate, void *stream);

/* out[i][c] = in[i][c] * mask[c]  (masked pose fed to smil_lbs_forward) */
int smil_mask_rows(const float *in, const float *mask, int64_t rows, int32_t cols, float *out, void *stream);

/* smil_prior_losses + the silhouette objective (objs[5] += sum_n pix_scale[n] * loss_img[n]; loss_img NULL to skip;
 * fitter.py:332-333) + the reduction of the per-image fov sums of smil_project_backward to d_fov (cam->nFov,),
 * overwritten (d_fov NULL to skip): the tail of one fit iteration in ONE launch. */
int smil_fit_epilogue(const SmilFitConfig *cfg, const float *pose, const float *trans, const float *betas,
                      const float *mean_betas, const float *betas_prec, const float *mask, const float *halo_prev,
                      const float *halo_next, float *objs, float *d_pose, float *d_trans, float *d_betas, int32_t accumulate,
                      const float *loss_img, const float *pix_scale, int32_t n_img, const SmilCameras *cam,
                      const float *d_fov_img, float *d_fov, void *stream);

/* 2-D joint loss (fitter.py:283,292-296).  proj / d_proj (N*views,J,2) in (y,x) px over ALL model joints;
 * canon (Jc,) = config.CANONICAL_MODEL_JOINTS (NULL: the first Jc joints); target (N*views,Jc,2);
 * visibility (N*views,Jc) int32.  objs[0] ADDED, d_proj overwritten. */
int smil_joint_loss(const SmilFitConfig *cfg, int32_t views, int32_t Jc, const int32_t *canon, const float *proj,
                    const float *target, const int32_t *visibility, float *objs, float *d_proj, void *stream);

/* The six loss terms of SMALFitter.forward (fitter.py:292-333) for every WINDOW of this shard separately, computed from the buffers
 * one whole-batch iteration left behind (proj from smil_lbs_forward_project / smil_project, loss_img from smil_silhouette_l1_fused,
 * objs_total = the iteration's objs after smil_fit_epilogue): what the reference's per-window forward() calls of one epoch return
 * (optimize_to_joints.py:153-157), without evaluating the windows one by one.  objs_win (n_windows,6), overwritten:
 * [joint, limit, pose, splay, betas, sil_reproj].  proj NULL: no joint term; loss_img NULL: no silhouette term.  The shard must start
 * at a window boundary and n_windows = ceil(N / window). */
int smil_window_terms(const SmilFitConfig *cfg, int32_t views, int32_t Jc, const int32_t *canon, const float *proj,
                      const float *target, const int32_t *visibility, const float *pose, const float *mask,
                      const float *objs_total, const float *loss_img, const float *pix_scale, float *objs_win,
                      int32_t n_windows, void *stream);

/* Helpers of the fused silhouette term: pix_scale[n] = w_reproj / (b_w views S^2); target_sum[n] =
 * sum_px |target[n]| (once per fit); objs[5] += sum_n pix_scale[n] loss_img[n]. */
int smil_pix_scale(const SmilFitConfig *cfg, int32_t views, int32_t S, float *pix_scale, void *stream);
int smil_image_abs_sum(const void *images, int32_t is_u8, int32_t N, int32_t pixels, float *out, void *stream);
int smil_sil_objective(const float *loss_img, const float *pix_scale, int32_t N, float *objs, void *stream);

/* torch.optim.Adam semantics (no amsgrad, no weight decay). step = 1-based step count.  The betas are double in all three entry
 * points: 1 - beta is formed in double from the value the caller wrote (1 - 0.999 = 0.001, as torch does) and then rounded to
 * float32, where 1.0f - 0.999f would be 1.3e-5 off.  Everything else, the bias corrections included, is float32 arithmetic. */
int smil_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                   float lr, double beta1, double beta2, float eps, int32_t step, void *stream);
/* The same update for up to SMIL_ADAM_MAX_TENSORS parameter tensors in ONE launch (a fit iteration updates five small
 * tensors; five launches cost more than the arithmetic).  Each tensor has its own learning rate and step count. */
#define SMIL_ADAM_MAX_TENSORS 8
typedef struct {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    int64_t n;
    float lr;
    int32_t step;             /* 1-based */
} SmilAdamTensor;
int smil_adam_step_multi(const SmilAdamTensor *tensors, int32_t count, double beta1, double beta2, float eps, void *stream);

/* Same update with the step count read from device memory: step = *step_dev - step_offset.  Lets a whole fit iteration be
 * captured once in a hipGraph and replayed (the host only bumps the counter - or the graph does, with an increment node). */
int smil_adam_step_dev(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                       float lr, double beta1, double beta2, float eps, const int32_t *step_dev, int32_t step_offset,
                       void *stream);

/* ------------------------------------------------------------------------------------------
 * 3-D scan registration losses (smilify_amd/csrc/mesh3d.hip).  Replace the pytorch3d 0.7.8 ops that the reference's
 * fitter_3d/trainer.py:3-9 imports and Stage.forward (:368-388) calls: sample_points_from_meshes, chamfer_distance,
 * mesh_edge_loss, mesh_normal_consistency, mesh_laplacian_smoothing(method="uniform").  Deterministic: two calls on the same
 * inputs give the same bits (no float atomics).
 * ---------------------------------------------------------------------------------------- */
/* sample_points_from_meshes (trainer.py:376): S points per mesh of N packed meshes.  verts (n_verts,3); faces (F_total,3) indices
 * into the packed verts; face_off (N+1) the first face of every mesh; cum_area (F_total) float64, the mesh's inclusive cumulative
 * face areas divided by its total (last entry 1; a mesh of zero area gives zero points).  Face ~ area, barycentrics of pytorch3d's
 * _rand_barycentric_coords, random numbers from Philox4x32-10 keyed by (seed, mesh, sample).  out (N,S,3); out_face (N,S) the
 * face index within its mesh, or NULL. */
int smil_sample_points(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, const double *cum_area,
                       int32_t N, int32_t S, uint64_t seed, float *out, int32_t *out_face, void *stream);

/* chamfer_distance(x, y) (trainer.py:379) with norm=2, no lengths or normals: x (N,P1,3), y (N,P2,3) ->
 * loss[0] = red_n [ red_i min_j |x_i - y_j|^2 + red_j min_i |y_j - x_i|^2 ], red = mean (or sum with point_sum / batch_sum); the
 * second half is dropped when single_directional.  idx_x (N,P1) / idx_y (N,P2): the argmin (smallest index on a tie) or NULL.
 * d_x (N,P1,3), d_y (N,P2,3): dloss/dx, dloss/dy (both or neither).  workspace: smil_chamfer_workspace_bytes. */
size_t smil_chamfer_workspace_bytes(int32_t N, int32_t P1, int32_t P2);
int smil_chamfer(const float *x, const float *y, int32_t N, int32_t P1, int32_t P2, int32_t single_directional, int32_t point_sum,
                 int32_t batch_sum, float *loss, int32_t *idx_x, int32_t *idx_y, float *d_x, float *d_y, void *workspace, void *stream);

/* Topology tables of one face array, built once by the caller and shared by B meshes (device pointers). */
typedef struct {
    int32_t V, E, Q;            /* vertices, unique edges, normal-consistency face pairs */
    const int32_t *edges;       /* (E,2) v0 < v1 (Meshes.edges_packed) */
    const int32_t *pairs;       /* (Q,4) (v0, v1, a, b): edge v0 v1 and the opposite vertices of two faces sharing it */
    const int32_t *nbr_ptr;     /* (V+1) Laplacian neighbour CSR: the edge neighbours of every vertex */
    const int32_t *nbr;         /* (2E) */
    const float *inv_deg;       /* (V) 1/deg, 0 for an isolated vertex */
    const int32_t *vpair_ptr;   /* (V+1) vertex -> pair incidence CSR */
    const int32_t *vpair;       /* (4Q) pair * 4 + role (0: v0, 1: v1, 2: a, 3: b) */
} SmilMeshTopology;
#define SMIL_REG_EDGE 1
#define SMIL_REG_NORMAL 2
#define SMIL_REG_LAPLACIAN 4
/* mesh_edge_loss / mesh_normal_consistency / mesh_laplacian_smoothing("uniform") (trainer.py:383-396) of B meshes verts (B,V,3) on one
 * topology: out3 = {edge, normal, laplacian} (each: per-mesh mean, then mean over meshes; terms not in the mask are 0).  d_edge,
 * d_normal, d_lap (B,V,3): the gradients of out3[0..2], or NULL.  workspace: smil_mesh_reg_workspace_bytes. */
size_t smil_mesh_reg_workspace_bytes(const SmilMeshTopology *t, int32_t B);
int smil_mesh_regularisers(const SmilMeshTopology *t, const float *verts, int32_t B, int32_t terms, float *out3, float *d_edge,
                           float *d_normal, float *d_lap, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * The SDF-guided term of the 3-D registration (reference fitter_3d/utils.py:973-1394, trainer.py:398-433): K nearest neighbours,
 * the term itself and the vertex sampler.  Deterministic like the functions above.
 * ---------------------------------------------------------------------------------------- */
#define SMIL_KNN_MAX_K 64
/* pytorch3d.ops.knn_points(x, y, K) with norm=2, no lengths: for every point of x (N,P1,3) its K nearest points of y (N,P2,3) by
 * squared distance, ascending by (distance, index): dists_x / idx_x (N,P1,K).  With dists_y / idx_y (N,P2,K) also y's points in x
 * (both or neither).  1 <= K <= SMIL_KNN_MAX_K and K <= the number of candidates.  After the call the first 8 bytes of the
 * workspace hold the number of list insertions as a uint64 (a measure of the search's work). */
size_t smil_knn_workspace_bytes(int32_t N, int32_t P1, int32_t P2, int32_t K);
int smil_knn(const float *x, const float *y, int32_t N, int32_t P1, int32_t P2, int32_t K, float *dists_x, int32_t *idx_x, float *dists_y,
             int32_t *idx_y, void *workspace, void *stream);

/* SDF_distance (utils.py:1127): with z the per-(mesh, side) z-scores of the values ((s - mean) / max(unbiased std, 1e-8)) and
 * (d_ik, j_ik) the K nearest candidates of query i, r_i = sum_k softmax_k(-|z_q[i] - z_c[j_ik]| / 0.1) d_ik;
 * loss[0] = red_n [ red_i r_i(x in y) + red_j r_j(y in x) ], red = mean (or sum with point_sum / batch_sum); the second half is dropped
 * when single_directional.  x (N,P1,3), y (N,P2,3), x_sdf (N,P1), y_sdf (N,P2); P1, P2 >= 2.  d_x, d_y: dloss/dx, dloss/dy (both
 * or neither; the values carry no gradient).  dists_x / idx_x (N,P1,K), dists_y / idx_y (N,P2,K): the neighbour tables, or NULL.
 * The first 8 bytes of the workspace: as smil_knn. */
size_t smil_sdf_distance_workspace_bytes(int32_t N, int32_t P1, int32_t P2, int32_t K);
int smil_sdf_distance(const float *x, const float *y, const float *x_sdf, const float *y_sdf, int32_t N, int32_t P1, int32_t P2, int32_t K,
                      int32_t single_directional, int32_t point_sum, int32_t batch_sum, float *loss, float *d_x, float *d_y,
                      float *dists_x, int32_t *idx_x, float *dists_y, int32_t *idx_y, void *workspace, void *stream);

/* sample_points_from_meshes_and_SDF (utils.py:1264): S vertices per mesh of N packed meshes, uniform with replacement.  verts
 * (n_verts,3) and values (n_verts) packed, vert_off (N+1) the first vertex of every mesh.  Sample s of mesh n takes word 0 of
 * Philox4x32-10 at counter (s, n, 1, 0) under the key (seed lo, seed hi) as r and the vertex (r * V_n) >> 32.  out (N,S,3),
 * out_values (N,S), out_idx (N,S) the vertex within its mesh (-1 and zeros for an empty mesh). */
int smil_sample_vertices(const float *verts, const float *values, const int32_t *vert_off, int32_t N, int32_t S, uint64_t seed, float *out,
                         float *out_values, int32_t *out_idx, void *stream);
/* Its gradient: d_verts (n_verts,3) = the sum of d_pts (N,S,3) over the samples that drew each vertex, in an order-independent
 * fixed-point sum.  max_verts: the largest mesh's vertex count. */
size_t smil_sample_vertices_backward_workspace_bytes(int32_t n_verts, int32_t N);
int smil_sample_vertices_backward(const float *d_pts, const int32_t *idx, const int32_t *vert_off, int32_t n_verts, int32_t max_verts,
                                  int32_t N, int32_t S, float *d_verts, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * The per-sample "spatial diameter" values that the SDF-guided term takes as input, by brute-force ray casting
 * (smilify_amd/csrc/raycast.hip).  Replaces compute_ray_mesh_intersections_vectorized (reference fitter_3d/SDF_tests.py:112-222) and
 * the ray / sample loops of compute_sdf (:344-382).  Deterministic: two calls on the same inputs give the same bits.
 * ---------------------------------------------------------------------------------------- */
/* S samples with R rays each against all F faces of one mesh: verts (V,3), faces (F,3), origins (S,3), own_face (S) the face a
 * sample lies on (never hit by its rays; -1: none), dirs (S,R,3) used as given (not normalised).  With e1 = v1 - v0, e2 = v2 - v0,
 * h = d x e2, a = e1 . h, f = 1 / a, s = o - v0, u = f (s . h), q = s x e1, v = f (d . q), t = f (e2 . q), face j is hit when
 * j != own_face, |a| > 1e-6, 0 <= u <= 1, v >= 0, u + v <= 1 and t > t_min, all in float32.  A ray's value is the LARGEST t over its
 * hits (the winning face's t, evaluated once more in float64 and rounded): ray_t (S,R), -1 where nothing is hit, or NULL.  diam (S):
 * the rays are walked in order, a ray is valid when it has a hit with d_lo < t < d_hi, the walk ends once `cap` (>= 1) valid rays
 * are taken; the mean of those as float32 (summed in float64), or d_lo when there are none.
 * t_min >= 0.  A face with a vertex index outside [0, V) is never hit.  workspace: smil_ray_diameters_workspace_bytes. */
size_t smil_ray_diameters_workspace_bytes(int32_t F, int32_t S, int32_t R);
int smil_ray_diameters(const float *verts, int32_t V, const int32_t *faces, int32_t F, const float *origins, const int32_t *own_face,
                       const float *dirs, int32_t S, int32_t R, float t_min, float d_lo, float d_hi, int32_t cap, float *ray_t,
                       float *diam, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * The PointNet++ set-abstraction operations of the point-cloud regressor (smilify_amd/csrc/pointnet2.hip).  Replace
 * farthest_point_sample, query_ball_point and the index_points + cat + permute grouping of the reference's
 * fitter_3d/pointcloud2smil/pointnet2_utils.py.  Deterministic: two calls on the same inputs give the same bits (no float atomics).
 * Every function checks its sizes before its pointers and both before it launches anything.
 * ---------------------------------------------------------------------------------------- */
#define SMIL_FPS_MAX_N 16384     /* points of one cloud in smil_fps: a cloud stays in the registers of one workgroup */
#define SMIL_BALL_MAX_RADII 4    /* (radius, nsample) pairs of one smil_ball_query call */
/* farthest_point_sample (pointnet2_utils.py:69-90): xyz (B,N,3), start (B) the first index of every cloud (the reference draws it
 * with torch.randint; clamped to [0, N)), out (B,npoint) int32.  out[b,0] = start[b]; the running distance starts at 1e10 and takes
 * d = (dx dx + dy dy) + dz dz (float32, every operation rounded on its own) where d < distance; the next index is the argmax of the
 * running distance, the SMALLEST index among equal maxima (so npoint > N or duplicate points give index 0 once every distance is
 * 0).  N > SMIL_FPS_MAX_N: SMIL_E_UNSUPPORTED. */
int smil_fps(const float *xyz, const int32_t *start, int32_t B, int32_t N, int32_t npoint, int32_t *out, void *stream);

/* query_ball_point (pointnet2_utils.py:93-113) at 1 .. SMIL_BALL_MAX_RADII radii in one pass: xyz (B,N,3) candidates, new_xyz
 * (B,S,3) queries; radii, nsample and out are HOST arrays of n_radii entries, out[r] a device array (B,S,K_r) int32 with
 * K_r = min(nsample[r], N).  A row holds the first K_r candidate indices, ascending, with d^2 <= r^2 (d^2 as in smil_fps,
 * r^2 = radius * radius formed in double and rounded once to float32; equality is inside, as the reference excludes only
 * sqrdists > radius ** 2), padded with the row's first hit; a query without a hit gets N in every slot. */
int smil_ball_query(const float *xyz, const float *new_xyz, int32_t B, int32_t N, int32_t S, int32_t n_radii, const double *radii,
                    const int32_t *nsample, int32_t *const *out, void *stream);

/* The grouped tensor a set-abstraction layer's Conv2d reads (pointnet2_utils.py:131-138 and :249-258), contiguous (B,C,K,S):
 * out[b,c,k,s] over the channels [xyz[b,i] - centres[b,s] (3), features[b,i] (D)] with i = idx[b,s,k] - or [features, xyz - centre]
 * when xyz_last (the two orders of sample_and_group and PointNetSetAbstractionMsg).  xyz (B,N,3) or NULL (no coordinate channels:
 * index_points), centres (B,S,3) or NULL (coordinates as they are), features (B,N,D) or NULL when D = 0, idx (B,S,K) int32.  An
 * index outside [0, N) gives zeros in every channel (the reference raises IndexError). */
int smil_group_points(const float *xyz, const float *centres, const float *features, const int32_t *idx, int32_t B, int32_t N, int32_t S,
                      int32_t K, int32_t D, int32_t xyz_last, float *out, void *stream);
/* Its gradient to the features: d_features (B,N,D) = the sum of d_out (B,C,K,S)'s feature channels over the (s,k) with
 * idx[b,s,k] = n, as an order-independent int64 fixed-point sum (unit from the cloud's largest |d_out| and K S addends); an index
 * outside [0, N) receives nothing.  has_xyz / xyz_last: the channel layout of the forward call.  The coordinates carry no gradient. */
size_t smil_group_points_backward_workspace_bytes(int32_t B, int32_t N, int32_t D);
int smil_group_points_backward(const float *d_out, const int32_t *idx, int32_t B, int32_t N, int32_t S, int32_t K, int32_t D,
                               int32_t has_xyz, int32_t xyz_last, float *d_features, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * Multi-view keypoint triangulation (smilify_amd/csrc/triangulate.hip).  Replaces the loop of triangulate_all and the functions it
 * calls in the reference's smal_fitter/sleap_data/triangulate_3d_points.py (:156-301, :830-978).  float64 throughout; one wave per
 * (frame, keypoint) problem; deterministic.  Sizes, limits and pointers are checked, in that order, before anything is launched.
 * ---------------------------------------------------------------------------------------- */
#define SMIL_TRI_MAX_VIEWS 32        /* cameras: the 2 C rows of a problem's system are the lanes of one wave */
#define SMIL_TRI_MAX_HYP 50          /* pair hypotheses of one problem (the reference's max_hypotheses) */
#define SMIL_TRI_RANSAC 1            /* mode bit: pair RANSAC where a problem has >= 3 valid views (use_ransac) */
#define SMIL_TRI_KEEP_ALL_VIEWS 2    /* mode bit: no view filter, every camera is a valid view (the single-point functions) */
/* P (C,3,4) projection matrices; K (C,3,3) and dist (C,5) = (k1,k2,p1,p2,k3), both or neither: with them the observations of a
 * camera whose coefficients are not all within 1e-8 of zero are undistorted first (normalise by fx, fy, cx, cy; five rounds of
 * x <- (x0 - tangential(x)) / radial(x); back through K).  obs (N,Kp,C,2) pixel (x, y), scores (N,Kp,C) or NULL.
 * A view is dropped when a coordinate is NaN, when its score is not NaN and < confidence_threshold, or when it is exactly (0, 0);
 * n views remain, numbered in camera order.  status (N,Kp): 0 triangulated, 1 n < min_views, 2 no hypothesis reached min_views
 * inliers.  mode & SMIL_TRI_RANSAC and n >= 3: the hypotheses are the pairs pairs[n][0 .. min(n (n - 1) / 2, SMIL_TRI_MAX_HYP))
 * (pairs: (SMIL_TRI_MAX_VIEWS + 1, SMIL_TRI_MAX_HYP, 2) int32 view numbers, row n for n views, made by the caller); each is
 * triangulated from its two views, a view is its inlier when the reprojection error is < reproj_threshold, the lowest-index
 * hypothesis of the largest count wins and its inliers are triangulated again.  Otherwise all n views are.  A triangulation is the
 * right singular vector X of the smallest singular value of the rows x P[2] - P[0], y P[2] - P[1]; xyz (N,Kp,3) = X[:3] / X[3]
 * (X[3] = 0 and non-finite values propagate by IEEE arithmetic), NaN for status != 0.  views_used (N,Kp): the views of the final
 * system (0 for status != 0); mean_err (N,Kp): the mean reprojection error of xyz over all n views; view_err (N,Kp,C) or NULL: the
 * error per camera, NaN for a dropped view; inlier_mask (N,Kp) or NULL: bit c set when camera c is in the final system;
 * obs_undistorted (N,Kp,C,2) or NULL: the points of the valid views as they enter the systems (dropped views are not written).
 * C > SMIL_TRI_MAX_VIEWS: SMIL_E_UNSUPPORTED.  min_views >= 1. */
int smil_triangulate(const double *P, const double *K, const double *dist, const double *obs, const double *scores, const int32_t *pairs,
                     int64_t N, int32_t Kp, int32_t C, double confidence_threshold, int32_t min_views, double reproj_threshold,
                     int32_t mode, double *xyz, int32_t *status, int32_t *views_used, double *mean_err, double *view_err,
                     uint32_t *inlier_mask, double *obs_undistorted, void *stream);

/* ------------------------------------------------------------------------------------------
 * Multi-view camera refinement (smilify_amd/csrc/refine.hip).  Replaces optimize_camera and reprojection_residuals of the reference's
 * smal_fitter/sleap_data/refine_camera_params.py (:143-226): every camera's parameters (rvec 3, t 3, fx, fy, cx, cy) are fitted to
 * its own 3-D / 2-D correspondences, all cameras in one call.  float64 throughout; deterministic (no atomics).
 * The cost is scipy's loss="soft_l1" on every scalar residual f (projected - observed, x and y): z = (f / f_scale)^2,
 * cost = 0.5 f_scale^2 sum 2 (sqrt(1 + z) - 1), weight w = 1 / sqrt(1 + z), g = J^T (w f), H = J^T diag(w) J with the analytic
 * Jacobian J.  The projection is u = fx x / z + cx, v = fy y / z + cy of (x, y, z) = Rodrigues(rvec) X + t; z <= 0 divides as IEEE does.
 * Correspondences are packed: camera c owns rows offsets[c] .. offsets[c + 1] of pts_3d (sum M, 3) and pts_2d (sum M, 2).  The
 * offset table (C + 1, int64) is passed twice, as a HOST array (checked here, sizes the launch) and as the same values on the device.
 * n_params = 6 fits rvec and t and keeps the four intrinsics of the initial parameters; 10 fits all.  Parameter arrays are (C,10).
 * Arguments are checked, in the order C, n_params, f_scale, offsets / workspace, monotone offsets, points, (max_steps), the other
 * pointers, before a device is touched.
 * ---------------------------------------------------------------------------------------- */
#define SMIL_REFINE_MIN_POINTS 20    /* a camera with fewer correspondences is skipped (reference :181-184) */
#define SMIL_REFINE_CONVERGED 0      /* status: an accepted step lowered the cost by < 1e-12 cost, or lambda passed 1e12 */
#define SMIL_REFINE_STEP_LIMIT 1     /*         max_steps evaluations without that */
#define SMIL_REFINE_SKIPPED 2        /*         fewer than SMIL_REFINE_MIN_POINTS correspondences: parameters returned unchanged */
#define SMIL_REFINE_NONFINITE 3      /*         the cost of the initial parameters is not finite: parameters returned unchanged */
size_t smil_refine_workspace_bytes(int32_t C, int64_t max_count); /* max_count: the largest correspondence count of a camera */
/* One accumulation at params (C,10): cost (C), g (C,10), H (C,10,10) symmetric; entries outside the n_params block are zero.  Every
 * camera is evaluated, whatever its count (none: zeros). */
int smil_refine_evaluate(const double *pts_3d, const double *pts_2d, const int64_t *offsets_host, const int64_t *offsets_dev, int32_t C,
                         const double *params, int32_t n_params, double f_scale, double *cost, double *g, double *H, void *workspace,
                         void *stream);
/* Levenberg-Marquardt from params0 (C,10).  THE RULES, which smil_refine_points below shares (one implementation,
 * smilify_amd/csrc/lm.h): lambda = 1e-3 at the start.  Every evaluation is of a candidate: accepted when its cost is finite and below
 * the current one (the candidate, its g and H are taken over, lambda <- max(lambda / 10, 1e-12)), else rejected (lambda <- 10 lambda);
 * the next candidate is current + delta with (H + lambda diag H) delta = -g by Cholesky.  A factorisation that fails (a pivot that is
 * not positive and finite) or a non-finite delta gives no step: lambda <- 10 lambda and the candidate is the current point, which the
 * next evaluation rejects.  Done when an accepted step lowered the cost by less than 1e-12 of it or when lambda > 1e12.  The first
 * evaluation is of the start itself and must be finite.
 * Here an evaluation is one enqueued (accumulate, step) pair over all cameras, at most max_steps of them; a done camera's later
 * launches do nothing.  Outputs per camera: params (C,10), status (SMIL_REFINE_*), n_accepted (accepted steps), n_trials
 * (evaluations, the first included), cost0 and cost (initial and final; NaN for a skipped camera), g (C,10) at params.
 * UNLIKE the rest of this header the call synchronises `stream`: it reads the done flags every 8 pairs and stops enqueuing once
 * every camera is done.  It must not be captured into a graph. */
int smil_refine_cameras(const double *pts_3d, const double *pts_2d, const int64_t *offsets_host, const int64_t *offsets_dev, int32_t C,
                        const double *params0, int32_t n_params, double f_scale, int32_t max_steps, double *params, int32_t *status,
                        int32_t *n_accepted, int32_t *n_trials, double *cost0, double *cost, double *g, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * Robust nonlinear refinement of triangulated points (smilify_amd/csrc/refine_points.hip).  AN EXTENSION: the reference has no such
 * function, its points stay the DLT points of triangulate_point_dlt.  Every (frame, keypoint) point is moved from xyz0 to the minimum
 * of the robust reprojection cost over its views, all points in one call: the point half of a bundle adjustment whose camera half is
 * smil_refine_cameras.  float64 throughout; one wave per problem; deterministic (no atomics), and a problem's result does not depend
 * on its place in the batch or on the batch size.
 * Inputs in the layouts smil_triangulate produces: P (C,3,4); obs (N,Kp,C,2) undistorted pixels (its obs_undistorted); view_mask
 * (N,Kp) with bit c set when camera c is a view of the problem (its inlier_mask; bits from C up are ignored); xyz0 (N,Kp,3).  The
 * observation of a view outside the mask is never read: it may be unwritten, NaN or garbage.  C <= SMIL_TRI_MAX_VIEWS.
 * For view c with h = P_c (X, 1) the two scalar residuals are f = (h0 / h2 - x, h1 / h2 - y) (h2 <= 0 divides as IEEE does) and their
 * Jacobian rows (P_c[k,:3] - (h_k / h2) P_c[2,:3]) / h2.  Cost, w, g = J^T (w f) and H = J^T diag(w) J are exactly those defined for
 * smil_refine_cameras above (scipy's soft_l1 on every scalar residual, the cost term written 2 z / (sqrt(1 + z) + 1)), with J 2n x 3.
 * Arguments are checked, in the order C, f_scale, N and Kp, (max_steps), the pointers, before a device is touched: C < 1, a
 * non-positive or non-finite f_scale, a negative N or Kp, max_steps < 1 or a null required pointer is SMIL_E_INVALID,
 * C > SMIL_TRI_MAX_VIEWS is SMIL_E_UNSUPPORTED; a call with N Kp = 0 succeeds and launches nothing.  Both entry points are asynchronous
 * on `stream` and need no workspace.
 * ---------------------------------------------------------------------------------------- */
#define SMIL_REFINE_POINTS_FEW_VIEWS 2 /* status: fewer than 2 views in the mask: xyz returned unchanged (0, 1 and 3 are SMIL_REFINE_CONVERGED,
                                          SMIL_REFINE_STEP_LIMIT and SMIL_REFINE_NONFINITE: a non-finite cost at xyz0, which includes a NaN
                                          xyz0 of a failed triangulation: xyz returned unchanged) */
/* One accumulation at xyz (N,Kp,3): cost (N,Kp), g (N,Kp,3), H (N,Kp,3,3) symmetric.  Every problem is evaluated, whatever its views
 * (none: zeros). */
int smil_refine_points_evaluate(const double *P, const double *obs, const uint32_t *view_mask, const double *xyz, int64_t N, int32_t Kp,
                                int32_t C, double f_scale, double *cost, double *g, double *H, void *stream);
/* Levenberg-Marquardt per problem under THE RULES stated at smil_refine_cameras (the same code, with a 3 x 3 system).  The first of
 * the at most max_steps evaluations is of xyz0.
 * UNLIKE smil_refine_cameras the loop runs INSIDE the kernel, bounded by max_steps: the problems are independent and there may be
 * millions of them, so nothing is gained by a launch per step, the call does not synchronise and it may be captured into a graph.
 * Outputs per problem: xyz (N,Kp,3), status, n_accepted (accepted steps), n_trials (evaluations, the first included; 0 for
 * SMIL_REFINE_POINTS_FEW_VIEWS), cost0 and cost (initial and final; NaN for SMIL_REFINE_POINTS_FEW_VIEWS), view_err (N,Kp,C) or NULL:
 * the reprojection error sqrt(f_x^2 + f_y^2) of the returned xyz per view of the mask, NaN for a view outside it. */
int smil_refine_points(const double *P, const double *obs, const uint32_t *view_mask, const double *xyz0, int64_t N, int32_t Kp, int32_t C,
                       double f_scale, int32_t max_steps, double *xyz, int32_t *status, int32_t *n_accepted, int32_t *n_trials,
                       double *cost0, double *cost, double *view_err, void *stream);

/* ------------------------------------------------------------------------------------------
 * Target image preparation (smilify_amd/csrc/imageprep.hip, smilify_amd/imageprep.py).  Replaces the host loops that make the
 * fitter's silhouette and RGB targets in the reference: cv2.undistort per frame (smal_fitter/sleap_data/
 * preprocess_sleap_multiview_dataset.py:710-735, :969-1028) and crop_to_silhouette (smal_fitter/utils.py:7-49: bounding box, 1.05 x
 * square, padding, cv2.resize).  No gradient, no workspace, asynchronous on `stream`; two calls give the same bits.
 * ---------------------------------------------------------------------------------------- */
/* sil (N,H,W), uint8 (sil_is_u8) or float32 -> bounds (N,5) int32 = y_min, y_max, x_min, x_max, count over the pixels > 0 (a NaN is
 * not); an image without one keeps H, -1, W, -1, 0.  Integer minima, maxima and sums only.  Pixels are indexed as int in slabs of 2^16:
 * H W <= 2^31 - 1 - 2^16 and N ceil(H W / 2^16) <= 2^31 - 1 (the grid) are required. */
int smil_image_bounds(const void *sil, int32_t sil_is_u8, int64_t N, int32_t H, int32_t W, int32_t *bounds, void *stream);

#define SMIL_WARP_EXACT 0          /* coordinate modes */
#define SMIL_WARP_RESIZE_LINEAR 1
#define SMIL_WARP_RESIZE_NEAREST 2
#define SMIL_WARP_NEAREST 0        /* interpolation */
#define SMIL_WARP_BILINEAR 1
/* One resampling of N output images of S_h x S_w pixels from N_src source images; output image n reads source image n % N_src and row
 * n % k of every table of k rows (k >= 1).  For output column j and row i, in float64 and without contraction:
 *   SMIL_WARP_EXACT           u = ax j + bx, v = ay i + by.  With a lens (K, K_new, dist all non-NULL; this mode only) these are pixels
 *                             of the camera K_new: x = (u - K_new[0][2]) / K_new[0][0], y = (v - K_new[1][2]) / K_new[1][1],
 *                             r2 = x x + y y, radial = 1 + k1 r2 + k2 r2^2 + k3 r2^3, xd = x radial + 2 p1 x y + p2 (r2 + 2 x x),
 *                             yd = y radial + p1 (r2 + 2 y y) + 2 p2 x y, and (u, v) <- (K[0][0] xd + K[0][2], K[1][1] yd + K[1][2])
 *                             (cv2.undistort / initUndistortRectifyMap as documented; skew and the other entries of K are not read).
 *                             nearest: the tap is floor(u + 0.5); bilinear: x0 = floor(u), fraction = float32(u - x0).
 *   SMIL_WARP_RESIZE_LINEAR   cv2.resize INTER_LINEAR: f = float32((j + 0.5) ax - 0.5), sx = floor(f), fraction = f - sx, and the
 *                             taps are (int)bx + sx and the next one: bx, by are the integral origin of the resized rectangle.
 *   SMIL_WARP_RESIZE_NEAREST  cv2.resize INTER_NEAREST: the tap is (int)bx + floor(j ax).
 * The interpolation of the two resize modes is their own.  A tap index is first clamped into clamp = (x_lo, x_hi, y_lo, y_hi)
 * (inclusive, source pixels; NULL: no clamp) - cv2.resize's edge replication, with the rectangle's last pixel as its min(.., side - 1)
 * - and a tap that then lies outside [0, W) x [0, H) reads border[c].  A non-finite u or v reads the border in every tap.
 * Bilinear: with the four taps a b / c d and the float32 fractions wx, wy: top = a + wx (b - a), bottom = c + wx (d - c),
 * value = top + wy (bottom - top), each operation rounded to float32 once (two equal taps give that tap exactly).  The value is
 * multiplied by `scale`.
 *   src      (N_src,H,W,C) channels-last, uint8 (src_is_u8) or float32; C in 1 .. 4
 *   out      (N,S_h,S_w,C), or with `planar` (N,C,S_h,S_w); float32, or with out_is_u8 uint8 = rint(min(max(value, 0), 255))
 *   affine   (n_affine,4) float64 = ax, bx, ay, by
 *   K, K_new (n_lens,3,3), dist (n_lens,5) = k1, k2, p1, p2, k3, float64; all three or none
 *   clamp    (n_clamp,4) int32 or NULL;  border (n_border,C) float32
 * Sizes, modes, table lengths and pointers are checked, and whatever cannot be indexed is refused, before anything is launched:
 * H, W < 2^30 (tap coordinates are int; the source itself is indexed with size_t, so H W is not bounded), S_h S_w <= 2^31 - 1 - 256
 * (an output pixel of one image is an int) and N ceil(S_h S_w / 256) <= 2^31 - 1 (the grid). */
typedef struct {
    const void *src;
    int32_t src_is_u8, N_src, H, W, C;
    void *out;
    int32_t out_is_u8, planar, N, S_h, S_w;
    int32_t coord_mode, interp;
    const double *affine; int32_t n_affine;
    const double *K, *K_new, *dist; int32_t n_lens;
    const int32_t *clamp; int32_t n_clamp;
    const float *border; int32_t n_border;
    float scale;
} SmilWarp;
int smil_warp_images(const SmilWarp *w, void *stream);

/* ------------------------------------------------------------------------------------------
 * Rotation conversions (smilify_amd/csrc/rotations.hip, rot.h; smilify_amd/rotations.py).  Replaces the four pytorch3d.transforms
 * functions of the reference's neural callers (smal_fitter/neuralSMIL/smil_image_regressor.py:26-96) and the matrices of its rotation
 * losses (:2123-2163, :3117-3266).  Arrays hold n rotations, contiguous, as 6 (6-D), 3 (axis-angle), 9 (matrix, row-major) or 1
 * (distance) values of the storage type `dtype`; all arithmetic is float64.  n == 0 succeeds without a launch; n < 0, a NULL required
 * pointer or an unknown dtype is SMIL_E_INVALID.  No workspace, asynchronous on `stream`.  A backward call takes the forward's INPUTS
 * and the upstream gradient and recomputes; it equals the first derivative of the formulas below with these conventions: the norm of
 * a zero vector has derivative 0, max(x, e) passes the gradient where x >= e, sqrt+ has derivative 0 where its argument is <= 0.
 *
 *   6-D -> matrix     a1 = d[0:3], a2 = d[3:6]; b1 = a1 / max(|a1|, 1e-12); u = a2 - (b1 . a2) b1; b2 = u / max(|u|, 1e-12); the rows
 *                     of R are b1, b2, b1 x b2.  Degenerate rows follow the formulas: zeros give the zero matrix.
 *   axis-angle -> matrix   theta = |a|; q = (cos(theta / 2), a s) with s = sin(theta / 2) / theta, continued to 1/2 at 0; with
 *                     q = (r, i, j, k) and t = 2 / (q . q):
 *                     R = [[1 - t (jj + kk), t (ij - kr), t (ik + jr)], [t (ij + kr), 1 - t (ii + kk), t (jk - ir)],
 *                          [t (ik - jr), t (jk + ir), 1 - t (ii + jj)]].
 *   matrix -> axis-angle   for any 3 x 3 m: qa = sqrt+ of (1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22,
 *                     1 - m00 - m11 + m22), sqrt+ x = sqrt(x) for x > 0, else 0.  Candidates (qa0^2, m21 - m12, m02 - m20, m10 - m01),
 *                     (m21 - m12, qa1^2, m10 + m01, m02 + m20), (m02 - m20, m10 + m01, qa2^2, m12 + m21),
 *                     (m10 - m01, m20 + m02, m21 + m12, qa3^2): the one of the largest qa (a tie: the lowest index), divided by
 *                     2 max(qa_c, 0.1), negated as a whole where its first entry is negative.  Then n = |q[1:]|, h = atan2(n, q0),
 *                     aa = q[1:] / (sin(h) / (2 h)), the divisor continued to 1/2 at h = 0.
 *   distance          dist = the Frobenius norm of R(p) - R(t) of two 6-D rotations; its gradient is 0 where dist == 0. */
#define SMIL_ROT_F32 0  /* dtype codes */
#define SMIL_ROT_F64 1
int smil_rot6d_to_matrix(const void *d6, void *R, int64_t n, int32_t dtype, void *stream);
int smil_rot6d_to_matrix_backward(const void *d6, const void *dR, void *dd6, int64_t n, int32_t dtype, void *stream);
int smil_axis_angle_to_matrix(const void *aa, void *R, int64_t n, int32_t dtype, void *stream);
int smil_axis_angle_to_matrix_backward(const void *aa, const void *dR, void *daa, int64_t n, int32_t dtype, void *stream);
int smil_matrix_to_axis_angle(const void *R, void *aa, int64_t n, int32_t dtype, void *stream);
int smil_matrix_to_axis_angle_backward(const void *R, const void *daa, void *dR, int64_t n, int32_t dtype, void *stream);
/* 6-D -> matrix -> axis-angle in one kernel, no matrix in memory.  Its backward is smil_matrix_to_axis_angle_backward at the matrix of
 * d6 followed by smil_rot6d_to_matrix_backward. */
int smil_rot6d_to_axis_angle(const void *d6, void *aa, int64_t n, int32_t dtype, void *stream);
/* dist (n).  The backward writes dp6 and / or dt6 (n,6); either may be NULL. */
int smil_rot6d_distance(const void *p6, const void *t6, void *dist, int64_t n, int32_t dtype, void *stream);
int smil_rot6d_distance_backward(const void *p6, const void *t6, const void *ddist, void *dp6, void *dt6, int64_t n, int32_t dtype,
                                 void *stream);

/* ------------------------------------------------------------------------------------------
 * Keypoint and triangulation losses of a multi-view regressor (smilify_amd/csrc/keypoint_losses.hip; smilify_amd/keypoint_losses.py).
 * Replaces the reference's smal_fitter/neuralSMIL/multiview_smil_regressor.py:1623-1838 (projection to views, damped DLT), :2250-2388
 * and :1050-1110 (the 2-D losses and the consistency term) and the per-sample loops of smil_image_regressor.py:3032-3115, :3334-3407.
 * Arrays are contiguous and hold the storage type `dtype` (SMIL_ROT_F32 / SMIL_ROT_F64); visibility and masks are bytes (non-zero:
 * true), joint weights and the work arrays are float64; all arithmetic is float64.  Empty sizes succeed; a negative size, a NULL
 * required pointer, an unknown dtype, flag or reduction is SMIL_E_INVALID.  Asynchronous on `stream`, no host synchronisation, no
 * atomics: every sum has a fixed order (lane-strided partials over the joints, a fixed butterfly over the wave, one workgroup over
 * the per-sample partials), so the same inputs give the same bits on every call.  A backward call takes the forward's INPUTS, what
 * the forward left in `factor`, and the upstream gradient as a DEVICE scalar or array; it recomputes the rest.
 *
 * (a) Squared error over pred, target (N,J,D), D = 2 or 3, eps = 1e-8.  Joint (n,j) is valid when mask[n] != 0 (mask (N) or NULL),
 *     vis[n,j] != 0 (vis (N,J) or NULL: visibility, or any explicit mask) and, by flag: SMIL_KP_TARGET_IN_UNIT every target
 *     coordinate lies in [0,1]; SMIL_KP_FINITE_NONZERO every prediction and target coordinate is finite and sum_d |t_d| > 0.
 *     With SMIL_KP_PRED_NAN_TO_ZERO a non-finite prediction coordinate counts as 0 and receives no gradient.  With weights w (J) or
 *     w = 1:  num_n = sum_j w_j valid_nj sum_d (p - t)^2,  count_n = sum_j w_j valid_nj.  Reductions:
 *       SMIL_KP_POOLED         sum_n num_n / (D sum_n count_n + eps) + eps;  with SMIL_KP_NO_TRAILING_EPS the same without the last
 *                              + eps, and exactly eps when no joint is valid
 *       SMIL_KP_VALID_SAMPLES  the mean of num_n / (D count_n + eps) over the samples with mask[n] != 0 that hold a valid joint, + eps
 *       SMIL_KP_SAMPLES        the same mean over all samples with mask[n] != 0, + eps
 *     (a mean over no sample is 0: with nothing valid every reduction is exactly eps.)  `partials` (N,4) is scratch, `factor` (N)
 *     receives d loss / d num_n, `loss` one value.  Backward: dpred = upstream factor_n 2 w_j valid_nj (p - t).
 * (b) Projection of joints (B,J,3) through cameras R (B,V,3,3), T (B,V,3), fov (B,V) in degrees, aspect (B,V) or NULL (1), image size
 *     S, to out (B,V,J,2): v = X R + T (row vectors); k11 = 1 / tan(fov pi / 360), k00 = k11 / aspect; x_ndc = k00 vx / vz,
 *     y_ndc = k11 vy / vz; (y, x) = (S/2 - S/2 y_ndc, S/2 - S/2 x_ndc) / (S + 1e-8), clamped to [0,1] - the camera of
 *     smilify_amd/csrc/camera.h in float64.  Backward: djoints, dR (all nine entries), dT, dfov, any of them NULL; a clamped
 *     coordinate passes its gradient where the unclamped value lies in [0,1], bounds included; none on aspect.
 * (c) (b) followed by (a) with D = 2, flags SMIL_KP_TARGET_IN_UNIT | SMIL_KP_PRED_NAN_TO_ZERO, reduction SMIL_KP_POOLED over the
 *     N = B V (sample, view) pairs with mask = view_mask (B,V); the projected array is never written.
 * (d) Damped DLT.  kp (B,V,J,2) normalised (y, x); for every (v,j) with vis[b,v,j] != 0 and view_mask[b,v] != 0 (either NULL: all):
 *     u = 1 - (x S) / (S / 2), v likewise from y; a1 = u [R[:,2]; T2] - k00 [R[:,0]; T0], a2 = v [R[:,2]; T2] - k11 [R[:,1]; T1];
 *     M = sum a_xyz a_xyz^T + damping I, c = -sum a_xyz a_w, points = M^-1 c (Cholesky).  valid (B,J): seen by >= 2 views; sane
 *     (B,J) or NULL: valid and |point| < max_norm.  Backward: lambda = M^-1 dpoints, dM = -lambda p^T, dc = lambda, through the rows
 *     to dR, dT, dfov (any NULL); lam_p (B,J,6) float64 is scratch.  The keypoints carry no gradient.  damping must be positive and
 *     finite (SMIL_E_INVALID otherwise): a joint seen by fewer than two views has a singular sum, and the damping is what keeps its
 *     factorisation, its point and its lambda finite. */
#define SMIL_KP_TARGET_IN_UNIT 1   /* flags of (a) */
#define SMIL_KP_PRED_NAN_TO_ZERO 2
#define SMIL_KP_FINITE_NONZERO 4
#define SMIL_KP_NO_TRAILING_EPS 8
#define SMIL_KP_POOLED 0           /* reductions of (a) */
#define SMIL_KP_VALID_SAMPLES 1
#define SMIL_KP_SAMPLES 2
int smil_kp_se_forward(const void *pred, const void *target, const uint8_t *vis, const uint8_t *mask, const double *weights, int64_t N,
                       int32_t J, int32_t D, int32_t flags, int32_t rule, int32_t dtype, double *partials, double *factor, void *loss,
                       void *stream);
int smil_kp_se_backward(const void *pred, const void *target, const uint8_t *vis, const uint8_t *mask, const double *weights,
                        const double *factor, const void *upstream, void *dpred, int64_t N, int32_t J, int32_t D, int32_t flags,
                        int32_t dtype, void *stream);
int smil_kp_project(const void *joints, const void *R, const void *T, const void *fov, const void *aspect, int64_t B, int32_t V, int32_t J,
                    double S, int32_t dtype, void *out, void *stream);
int smil_kp_project_backward(const void *joints, const void *R, const void *T, const void *fov, const void *aspect, const void *dout,
                             int64_t B, int32_t V, int32_t J, double S, int32_t dtype, void *djoints, void *dR, void *dT, void *dfov,
                             void *stream);
int smil_kp_project_loss(const void *joints, const void *R, const void *T, const void *fov, const void *aspect, const void *target,
                         const uint8_t *vis, const uint8_t *view_mask, const double *weights, int64_t B, int32_t V, int32_t J, double S,
                         int32_t dtype, double *partials, double *factor, void *loss, void *stream);
int smil_kp_project_loss_backward(const void *joints, const void *R, const void *T, const void *fov, const void *aspect, const void *target,
                                  const uint8_t *vis, const uint8_t *view_mask, const double *weights, const double *factor,
                                  const void *upstream, int64_t B, int32_t V, int32_t J, double S, int32_t dtype, void *djoints, void *dR,
                                  void *dT, void *dfov, void *stream);
int smil_kp_triangulate(const void *kp, const uint8_t *vis, const uint8_t *view_mask, const void *R, const void *T, const void *fov,
                        const void *aspect, int64_t B, int32_t V, int32_t J, double S, double damping, double max_norm, int32_t dtype,
                        void *points, uint8_t *valid, uint8_t *sane, void *stream);
int smil_kp_triangulate_backward(const void *kp, const uint8_t *vis, const uint8_t *view_mask, const void *R, const void *T, const void *fov,
                                 const void *aspect, const void *dpoints, int64_t B, int32_t V, int32_t J, double S, double damping,
                                 int32_t dtype, double *lam_p, void *dR, void *dT, void *dfov, void *stream);

/* ------------------------------------------------------------------------------------------
 * Rigid and similarity alignment of 3-D keypoint sets (smilify_amd/csrc/align.hip, align.h; smilify_amd/align.py): the rotation R,
 * translation t and scale s that carry src (B,J,3) onto dst (B,J,3), dst_i ~ s R src_i + t, in the weighted least-squares sense, by
 * Horn's quaternion method.  An extension: the reference has no alignment; only the masking rule of its MPJPE is mirrored
 * (smal_fitter/neuralSMIL/benchmark_model.py:287-297).  Arrays are contiguous and hold the storage type `dtype` (SMIL_ROT_F32 /
 * SMIL_ROT_F64); weights, the saved records and the final weights are float64, masks are bytes (non-zero: true), the status is int32;
 * all arithmetic is float64 and every output is rounded once.  B == 0 succeeds without a launch; a negative size, a NULL required
 * pointer, an unknown dtype or mode, a min_gap that is negative or not finite, or (robust_iters > 0) a robust_scale that is not
 * positive and finite is SMIL_E_INVALID.  Asynchronous on `stream`, no host synchronisation, no atomics: one wave holds one problem
 * and sums its joints in a fixed order, so the same inputs give the same bits on every call.  No cap on B or J.
 *
 * Weights.  w_i = weights[i] (weights (J) with weight_rows == 0, (B,J) with 1, NULL: 1) where mask[b,i] != 0 (mask (B,J) or NULL), and
 *     0 where a coordinate of either point is not finite or the weight is not a positive finite number.  A joint of weight 0 is not
 *     read into any sum.
 * Moments, in two passes.  W = sum w, mx = sum w src / W, my = sum w dst / W; on x = src - mx, y = dst - my:
 *     M[a][b] = sum w x_a y_b, vx = sum w |x|^2.
 * Solve.  N (4 x 4, symmetric) from S = M: row 0 (Sxx+Syy+Szz, Syz-Szy, Szx-Sxz, Sxy-Syx), row 1 from the diagonal (Sxx-Syy-Szz,
 *     Sxy+Syx, Szx+Sxz), row 2 (-Sxx+Syy-Szz, Syz+Szy), row 3 (-Sxx-Syy+Szz).  Cyclic Jacobi, at most 12 sweeps, ended when the
 *     off-diagonal sum of squares is <= (2^-52 |N|_F)^2, gives lam_1 >= ... >= lam_4 and v_k; q = v_1 = (a,b,c,d) and
 *     R = [[aa+bb-cc-dd, 2(bc-ad), 2(bd+ac)], [2(bc+ad), aa-bb+cc-dd, 2(cd-ab)], [2(bd-ac), 2(cd+ab), aa-bb-cc+dd]]: even in q and
 *     always a proper rotation, a mirrored dst included.  s = sum_ab R[a][b] M[b][a] / vx with with_scale, else 1;  t = my - s R mx;
 *     gap = (lam_1 - lam_2) / max(lam_1, -lam_4);  rms = sqrt(sum w |s R x - y|^2 / W), summed over the joints.
 * Status.  SMIL_ALIGN_EMPTY where W == 0 (J == 0 included): R = I, s = 1, t = 0, gap = rms = 0.  SMIL_ALIGN_DEGENERATE where W > 0 and
 *     (vx == 0, or max |lam| == 0, or gap <= min_gap) - one point, two points, collinear or coincident points do not determine a
 *     rotation: R = I, s = 1, t = my - mx, gap as computed (0 for max |lam| == 0), rms of that transform.  Else SMIL_ALIGN_OK.  The
 *     gradients of a problem that is not SMIL_ALIGN_OK are exactly 0.
 * Robust variant.  robust_iters > 0 re-solves that many times, each with w_i = w0_i / sqrt(1 + r_i^2 / robust_scale^2),
 *     r_i = |s R src_i + t - dst_i| under the transform of the solve before (soft-L1, the cost of the refinement kernels).  The
 *     outputs are those of the last solve; w_final (B,J) or NULL receives its weights.
 * Backward, of an SMIL_ALIGN_OK problem, from gR (B,9), gt (B,3), gs (B) (any NULL: zero; gs is ignored without with_scale), with the
 *     weights of the last solve as constants; gap and rms carry no gradient.
 *       g_my = gt;  gs += -gt . (R mx);  gR += -s gt mx^T;  g_mx = -s R^T gt
 *       with_scale:  gR += gs M^T / vx;  gM = gs R^T / vx;  g_vx = -gs s / vx
 *       gq = 2 N(gR^T) q   (sum gR R(q) is the quadratic form q^T N(gR^T) q)
 *       u = sum_{k=2..4} v_k (v_k . gq) / (lam_1 - lam_k);  G = u q^T;  gM[a][b] += sum_ij G[i][j] dN[i][j] / dM[a][b]
 *       d src_i = w_i (gM y_i + 2 g_vx x_i) + (w_i / W) g_mx;   d dst_i = w_i gM^T x_i + (w_i / W) g_my
 *     (the centring terms cancel: sum w x = sum w y = 0).  `saved` (B, SMIL_ALIGN_SAVED) float64 is written by the forward (NULL: not
 *     kept) and read, with `status` and `w_final`, by the backward; dsrc and ddst may each be NULL.
 * Errors.  smil_align_errors: valid[b,i] = mask != 0, both points finite and, with `sentinel`, |target_i| > 1e-6; the alignment
 *     `mode` (SMIL_ALIGN_NONE: the identity) carries pred onto target with `valid` as weights; dist[b,i] = scale |s R pred_i + t -
 *     target_i|, 0 where the joint is not valid.  A sample that is not SMIL_ALIGN_OK uses the transform stated above and reports its
 *     status; with SMIL_ALIGN_NONE the status is SMIL_ALIGN_OK where a joint is valid, else SMIL_ALIGN_EMPTY.  Forward only. */
#define SMIL_ALIGN_OK 0          /* status */
#define SMIL_ALIGN_DEGENERATE 1
#define SMIL_ALIGN_EMPTY 2
#define SMIL_ALIGN_NONE 0        /* modes of smil_align_errors */
#define SMIL_ALIGN_RIGID 1
#define SMIL_ALIGN_SIMILARITY 2
#define SMIL_ALIGN_SAVED 40      /* float64 values the forward keeps per problem */
int smil_align_forward(const void *src, const void *dst, const double *weights, int32_t weight_rows, const uint8_t *mask, int64_t B,
                       int32_t J, int32_t with_scale, double min_gap, int32_t robust_iters, double robust_scale, int32_t dtype, void *R,
                       void *t, void *s, int32_t *status, void *gap, void *rms, double *w_final, double *saved, void *stream);
int smil_align_backward(const void *src, const void *dst, const double *w_final, const double *saved, const int32_t *status, const void *gR,
                        const void *gt, const void *gs, int64_t B, int32_t J, int32_t with_scale, int32_t dtype, void *dsrc, void *ddst,
                        void *stream);
int smil_align_errors(const void *pred, const void *target, const uint8_t *mask, int64_t B, int32_t J, int32_t mode, int32_t sentinel,
                      double scale, double min_gap, int32_t dtype, void *dist, uint8_t *valid, int32_t *status, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mesh-free joint kinematics (smilify_amd/csrc/joints.hip; tables: smilify_amd/joints.py).  The posed joints SMAL.__call__ returns
 * (smal_torch.py:340-351) without forming a vertex, for models WITHOUT pose blend shapes: a static-joint model's joints are the
 * translation column of the kinematic chain (J_transformed); a regressor model's are sum_k A_k m[j,k] over the (joint, bone) pairs
 * with a non-zero weight product, with the moments m = M0 + sum_b beta_b MB_b and the rest joints J_rest = J0 + sum_b beta_b JB_b
 * affine in the shape.  One wavefront per frame; all arithmetic is float64 on float32 parameters and every output is rounded once.
 * The semantics of the chain are those of smil_lbs_forward, stated in csrc/chain.h (Rodrigues with |theta + 1e-8|, the root's rotation-only rule, the y flip of
 * betas_trans, propagate_scaling, allow_limb_scaling, theta_mask).  No float atomics: two calls on the same inputs return the same
 * bits, the sums over frames of the shared tables' gradients included.
 * ---------------------------------------------------------------------------------------- */
typedef struct {                /* DEVICE pointers; built on the host in float64 once per model */
    int32_t J, nB, P;           /* joints, shape directions, (joint, bone) pairs (0 for a static-joint model) */
    int32_t max_depth;          /* deepest level of the chain */
    int32_t static_joints;
    const int32_t *parents;     /* (J) parents[0] = -1, parents[i] < i */
    const int32_t *depth;       /* (J) */
    const int32_t *child_ptr;   /* (J+1) children of every joint, ascending ... */
    const int32_t *child;       /* (J-1) ... gathered by the reverse walk in this order */
    const double *J0;           /* (J,3) rest joints of the template (J_static for a static-joint model) */
    const double *JB;           /* (nB,J,3) their shape directions */
    const int32_t *pair_ptr;    /* (J+1) pairs by joint */
    const int32_t *pair_bone;   /* (P) */
    const double *M0;           /* (P,4) moment of the template; [3] = sum_v Jreg[j,v] w[v,k] */
    const double *MB;           /* (P,nB,3) */
    const int32_t *bpair_ptr;   /* (J+1) the same pairs by bone */
    const int32_t *bpair_joint; /* (P) */
    const int32_t *bpair_index; /* (P) the entry's pair in the by-joint order (index into M0 / MB) */
    const double *rowsum;       /* (J) sum_v Jreg[j,v]: factor of a translation added before the regression */
} SmilJointTables;

typedef struct {                /* SmilLbsInputs without del_v, v_template and Rs_in; same conventions */
    int32_t B;
    int32_t shared_beta;
    int32_t nB_used;            /* 0 .. nB */
    const float *beta;          /* (B,nB_used) or (nB_used,); may be NULL when nB_used == 0 */
    const float *theta;         /* (B,J,3) axis-angle */
    const float *logscale;      /* (B,J,3) / (J,3) / NULL */
    int32_t logscale_shared;
    const float *btrans;        /* same conventions */
    int32_t btrans_shared;
    const float *trans;         /* (B,3) or NULL */
    int32_t trans_after_joints; /* 1: trans is added to the joints (fitter convention, static-joint models included); 0: SMAL.__call__ -
                                   trans is added to the vertices before the regression (times rowsum[j]) and a static-joint model's
                                   joints carry no trans at all (smal_torch.py:343-346) */
    int32_t propagate_scaling;
    int32_t allow_limb_scaling;
    const float *theta_mask;    /* (J,3) or NULL; d_theta is the gradient with respect to the MASKED pose */
} SmilJointsInputs;

/* joints (B,J,3) out; new_J (B,J,3) = SMAL.J_transformed, or NULL. */
int smil_joints_forward(const SmilJointTables *t, const SmilJointsInputs *in, float *joints, float *new_J, void *stream);

typedef struct {
    const float *d_joints;  /* (B,J,3) upstream gradient */
    float *d_beta;          /* (B,nB_used) or (nB_used,) when shared; NULL to skip (ignored when nB_used == 0) */
    float *d_theta;         /* (B,J,3); NULL to skip */
    float *d_trans;         /* (B,3); NULL to skip; zeros when `trans` has no effect on the joints */
    float *d_logscale;      /* (B,J,3) or (J,3) when shared; NULL to skip; zeros without logscale / allow_limb_scaling */
    float *d_btrans;        /* same; zeros without btrans */
    void *workspace;        /* smil_joints_backward_workspace_bytes: required iff a SHARED table's gradient is asked for.  Its first 256
                               bytes (the counter of finished blocks) must be zero before the first use; every call leaves them zero.
                               One workspace serves the calls of one stream */
} SmilJointsGrads;
/* Every output is overwritten.  The forward is recomputed in LDS: nothing is saved between the calls.  Gradients of shared tables
 * (shared beta, logscale, btrans) are sums over frames: every frame leaves its float64 row in the workspace and the rows are added in a
 * fixed order (runs of 256 frames, then runs of 256 partial sums, ...), rounded to float32 once. */
size_t smil_joints_backward_workspace_bytes(const SmilJointTables *t, const SmilJointsInputs *in, const SmilJointsGrads *g);
int smil_joints_backward(const SmilJointTables *t, const SmilJointsInputs *in, const SmilJointsGrads *g, void *stream);

/* ------------------------------------------------------------------------------------------
 * 3-D keypoint term on the mesh-free joints, fused: forward, term and backward of a frame in one launch (no (N,J,3) round trip).
 * With windows as everywhere in fit.hip (b_w frames in window w, from cfg->window, frame0, N_total; cfg->N frames, cfg->J joints;
 * cfg is not changed):
 *   objs[9] += w_k3d sum_w 1/(3 Jc b_w) sum_{n in w} sum_c vis[n,c] wj[c] rho(|joints[n,canon[c]] - target[n,c]|^2)
 * rho(s) = s when robust_scale == 0 (the 3-D twin of fitter.py:292-296), rho(s) = 2 sigma^2 (sqrt(1 + s / sigma^2) - 1) with
 * robust_scale = sigma > 0 (the soft-L1 of the refinement kernels).  A target row that is exactly (0,0,0) or holds a non-finite entry is
 * invisible; a frame with nothing visible contributes exactly 0 and gets exactly zero gradients.  The joints follow the fitter
 * convention (in->trans_after_joints must be 1); in->B must equal cfg->N.
 * canon (Jc) int32 joint ids (NULL: the first Jc joints), target (N,Jc,3) float32, visibility (N,Jc) uint8 or NULL, joint_weights (Jc)
 * float64 or NULL.  The RAW gradients are written (overwritten): d_pose (N,J,3) with respect to the masked pose, d_trans (N,3),
 * d_betas / d_logscale / d_btrans with the shapes of SmilJointsGrads (each may be NULL), so that smil_prior_losses(..., accumulate = 1)
 * run after it finishes them.  joints_out (N,J,3) or NULL.  workspace: smil_kp3d_fit_eval_workspace_bytes (the counter and the
 * per-block rows of the shared tables' gradients and of the term, zeroed like SmilJointsGrads.workspace; all sums over frames are
 * taken in a fixed order). */
size_t smil_kp3d_fit_eval_workspace_bytes(const SmilJointTables *t, const SmilJointsInputs *in, int32_t want_betas, int32_t want_logscale,
                                          int32_t want_btrans);
int smil_kp3d_fit_eval(const SmilFitConfig *cfg, double w_k3d, double robust_scale, const SmilJointTables *t, const SmilJointsInputs *in,
                       int32_t Jc, const int32_t *canon, const float *target, const uint8_t *visibility, const double *joint_weights,
                       float *objs, float *d_pose, float *d_trans, float *d_betas, float *d_logscale, float *d_btrans, float *joints_out,
                       void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * Multi-view 2-D keypoint term on the mesh-free joints, fused like smil_kp3d_fit_eval: chain, joints, projection into every view, the
 * term and the whole backward of a frame in one launch.  Images are numbered frame * views + view; cam->N = cfg->N * cam->views,
 * cam->views <= 64, cam->S the side of the square image the pixels are measured in.  With yx(X; cam) the (y, x) pixel position of a
 * world point and b_w the window sizes of smil_kp3d_fit_eval:
 *   objs[0] += w_k2d sum_w 1/(2 Jc Nv b_w) sum_{n in w} sum_{v < Nv} sum_{c < Jc}
 *              seen[n,v,c] conf[n,v,c] wj[c] rho(|yx(joints[n,canon[c]]; cam(n,v)) - target2d[n,v,c]|^2)
 * rho(s) = s when robust_scale_px == 0: with no confidences and no joint weights the value of smil_joint_loss on the same
 * projections, element for element (an unseen entry counts in the denominator: fitter.py:292-296); with robust_scale_px = sigma > 0
 * the soft-L1 2 sigma^2 (sqrt(1 + s / sigma^2) - 1), evaluated as 2 s / (1 + u), u = sqrt(1 + s / sigma^2), gradient factor 1 / u.
 * Camera arithmetic: that of csrc/camera.h in float64 on the float32 tables - X_view = X R + T; k11 = 1 / tan(fov / 2) (fov in
 * degrees), k00 = k11 / aspect; x_ndc = k00 x_view / z_view + px, y_ndc = k11 y_view / z_view + py (the principal point added after
 * the division); y_s = S/2 - (S/2) y_ndc, x_s = S/2 - (S/2) x_ndc.  R, T, fov, aspect and principal may each hold 1, views or
 * N * views rows, indexed image % rows.  The cameras are constants: no gradient on them is returned.
 * seen[n,v,c] holds iff visibility2d (if given) is non-zero, both target coordinates are finite, the confidence (if given) is finite
 * and > 0, and z_view of the joint in that camera (float64) is > SMIL_ZNEAR = 0.001.  An entry that is not seen contributes exactly 0
 * and no gradient.
 * The 3-D term of smil_kp3d_fit_eval (objs[9], its own visibility rule, the same joint_weights) is evaluated in the same launch when
 * target3d is not NULL and w_k3d > 0; the 2-D term when target2d is not NULL and w_k2d > 0; both add into the gradient on the joints
 * before the chain backward; a call that asks for neither is an error, and the slot of a term not asked for is not written.  A
 * frame with no seen entry in any view and no visible 3-D target contributes exactly 0 and writes +0 in every gradient.
 * target2d (N,Nv,Jc,2) float32 (y,x); visibility2d (N,Nv,Jc) uint8 or NULL; confidence (N,Nv,Jc) float32 or NULL; joint_weights
 * (Jc) float64 or NULL; target3d (N,Jc,3) / visibility3d (N,Jc) as in smil_kp3d_fit_eval, or NULL.  The gradient outputs, joints_out
 * and the workspace are those of smil_kp3d_fit_eval (RAW gradients, finished by smil_prior_losses(accumulate = 1)).  yx_out
 * (N,Nv,Jc,2) float32 or NULL: the projections of the canonical joints, rounded once, NaN where the depth rule fails (whatever the
 * targets hold).  Each lane adds its joint's contributions in a fixed order (the 3-D entries of the joint, then the 2-D ones: canon
 * entries ascending, views ascending within each); all sums over frames are taken in a fixed order: two calls return the same bits.
 * Errors (smil_last_error): a NaN, infinite or negative weight or scale; views outside 1..64; cam->N != cfg->N * views;
 * in->B != cfg->N; trans_after_joints != 1; a camera table whose row count is not 1, views or N * views. */
size_t smil_kp2d_fit_eval_workspace_bytes(const SmilJointTables *t, const SmilJointsInputs *in, const SmilCameras *cam, int32_t want_betas,
                                          int32_t want_logscale, int32_t want_btrans);
int smil_kp2d_fit_eval(const SmilFitConfig *cfg, double w_k2d, double robust_scale_px, const SmilJointTables *t, const SmilJointsInputs *in,
                       const SmilCameras *cam, int32_t Jc, const int32_t *canon, const float *target2d, const uint8_t *visibility2d,
                       const float *confidence, const double *joint_weights, double w_k3d, double robust_scale, const float *target3d,
                       const uint8_t *visibility3d, float *objs, float *d_pose, float *d_trans, float *d_betas, float *d_logscale,
                       float *d_btrans, float *joints_out, float *yx_out, void *workspace, void *stream);

/* smil_adam_step_multi with the bias corrections formed in double, as torch.optim.Adam forms them: 1 - beta1^step and
 * sqrt(1 - beta2^step) are computed in double from the betas the caller wrote and rounded to float32 once, and the step size
 * lr / (1 - beta1^step) likewise.  smil_adam_step_multi forms 1 - beta2^step in float32, which is up to 1e-5 off in its square root
 * for small step counts: every update is then that fraction of lr off, whatever the parameter's magnitude (2e-7 after five steps at
 * lr = 5e-3) - more than the rounding of parameters well below 1, which KeypointFitter3D's are.  Everything else is the float32
 * arithmetic of smil_adam_step_multi (csrc/fit.hip). */
int smil_adam_step_multi_bc64(const SmilAdamTensor *tensors, int32_t count, double beta1, double beta2, float eps, void *stream);

/* ------------------------------------------------------------------------------------------
 * Visual hull: multi-view voxel carving from silhouette masks (smilify_amd/csrc/visual_hull.hip, smilify_amd/visual_hull.py).  An
 * extension: the reference has no counterpart.  A point belongs to the hull if it projects onto foreground in the views that see
 * it.  No gradient; asynchronous on `stream`; pure gathers and integer reductions: two calls give the same bits.
 *
 * Camera arithmetic: exactly that of smil_kp2d_fit_eval ("Camera arithmetic" above) - float64 on the float32 SmilCameras tables,
 * y_s = S/2 - (S/2) y_ndc, x_s likewise, S = cam->S; tables of 1, views or N * views rows indexed image % rows, image =
 * frame * views + view; cam->N = N * views, views <= SMIL_HULL_MAX_VIEWS.  masks (N,views,H,W), uint8 or float32 (masks_f32): pixel
 * (r, c) covers [r, r+1) x [c, c+1) in (y_s, x_s); H x W need not be S x S (with opencv_to_pinhole_camera(..., S) the screen
 * coordinates are source pixels for any S).  View v SEES a point iff z_view > SMIL_ZNEAR = 0.001f, 0 <= y_s < H and 0 <= x_s < W, all
 * decided in float64 before any conversion to an integer (a NaN or infinite coordinate is not seen); it is IN FRONT iff z_view >
 * SMIL_ZNEAR.  A seen point is foreground in v iff mask[floor(y_s), floor(x_s)] > threshold (compared as float32; a NaN is
 * background).  fg = the views in which the point is seen and foreground; seen = the views that see it, or, with outside_carves != 0,
 * the views it is in front of (one that does not see it is then a miss).
 *
 * The grid: frame n's voxel (i, j, k), i < Gx fastest, has the linear index i + Gx (j + Gy k) and the centre
 * origin[n % n_origin] + ((i, j, k) + 0.5) * voxel_size[n % n_voxel_size], each coordinate formed in float64 as written (a product
 * and a sum, no fused multiply-add).  origin (n_origin,3) and voxel_size (n_voxel_size) are HOST arrays of 1 or N rows (they are
 * validated on the host and uploaded into the workspace by the calls that read them); everything else is device memory.
 * Gx Gy Gz <= 2^40; N * Gx * Gy * Gz may exceed 2^31: every index is 64-bit.
 * ---------------------------------------------------------------------------------------- */
#define SMIL_HULL_MAX_VIEWS 64
#define SMIL_HULL_STATS 16
typedef struct {
    int32_t N;                /* frames */
    int32_t Gx, Gy, Gz;       /* voxels per axis, each >= 1 */
    const double *origin;     /* HOST (n_origin,3): the grid's corner (NOT the first centre) */
    int32_t n_origin;         /* 1 or N */
    const double *voxel_size; /* HOST (n_voxel_size): the edge of a voxel, positive and finite */
    int32_t n_voxel_size;     /* 1 or N */
} SmilHullGrid;

/* occ (N,Gz,Gy,Gx) uint8 = seen >= min_views && seen - fg <= max_misses at every voxel centre; fg, seen (N,Gz,Gy,Gx) uint8: the
 * counts, or NULL.  workspace: smil_hull_carve_workspace_bytes(g) bytes of device memory.  Errors (smil_last_error): views outside
 * 1..64; cam->N != N * views; a camera table whose row count is not 1, views or N * views; a voxel_size that is not positive and
 * finite; a non-finite origin; a grid extent < 1; min_views outside 0..views; max_misses < 0; a NaN threshold; NULL masks, occ or
 * workspace. */
size_t smil_hull_carve_workspace_bytes(const SmilHullGrid *g);
int smil_hull_carve(const SmilHullGrid *g, const void *masks, int32_t masks_f32, int32_t H, int32_t W, float threshold,
                    const SmilCameras *cam, int32_t min_views, int32_t max_misses, int32_t outside_carves, uint8_t *occ, uint8_t *fg,
                    uint8_t *seen, void *workspace, void *stream);
/* The same test at arbitrary points (N,P,3) float32 (converted to float64): fg, seen (N,P) uint8. */
int smil_hull_query(const float *points, int32_t N, int64_t P, const void *masks, int32_t masks_f32, int32_t H, int32_t W, float threshold,
                    const SmilCameras *cam, int32_t outside_carves, uint8_t *fg, uint8_t *seen, void *stream);
/* stats (N,16) int64 over the voxels with occ != 0: count; sum i, sum j, sum k; sum i^2, sum j^2, sum k^2, sum ij, sum ik, sum jk;
 * min i, min j, min k; max i, max j, max k.  An empty frame keeps the minima Gx, Gy, Gz and the maxima -1 (as smil_image_bounds).
 * Exact integers (the grid must keep Gx Gy Gz max(G)^2 below 9e18).  g->origin and g->voxel_size are not read. */
int smil_hull_stats(const SmilHullGrid *g, const uint8_t *occ, int64_t *stats, void *stream);
/* The surface: the occupied voxels with an unoccupied 6-neighbour (the grid's border counts as unoccupied).
 * smil_hull_surface_count fills offsets (N+1) int64 - frame n's surface voxels are rows offsets[n] .. offsets[n+1] of the packed
 * output - and leaves per-workgroup prefixes in the workspace (smil_hull_surface_workspace_bytes(g) bytes; the table SIZES of g lay
 * it out, the tables are not read).  smil_hull_surface_write, with the SAME g, occ and workspace, stores the centres, rounded once
 * to float32, in points (offsets[N],3) and, if index is not NULL, the linear voxel indices in index (offsets[N]) int64: frames in
 * order and ascending linear index within a frame, whatever the scheduling.  The caller reads offsets[N] in between to size the
 * outputs (and skips the write when it is 0). */
size_t smil_hull_surface_workspace_bytes(const SmilHullGrid *g);
int smil_hull_surface_count(const SmilHullGrid *g, const uint8_t *occ, int64_t *offsets, void *workspace, void *stream);
int smil_hull_surface_write(const SmilHullGrid *g, const uint8_t *occ, void *workspace, float *points, int64_t *index, void *stream);

/* ------------------------------------------------------------------------------------------
 * Distance fields: the exact Euclidean distance transform of an occupancy grid (or of a batch of 2-D masks: Gz = 1, every image a
 * frame of grid (W, H, 1)) and a differentiable sampler of the field (smilify_amd/csrc/distance_field.hip).  An extension: the
 * reference has no counterpart.  Asynchronous on `stream`, no atomics, no host synchronisation; two calls give the same bits.
 *
 * The transform.  The feature set F of frame n is its voxels with occ != 0 (invert != 0: with occ == 0).
 * d2[n,k,j,i] = min over (i',j',k') in F of (i-i')^2 + (j-j')^2 + (k-k')^2: an int32 in voxel units, in the layout of occ, centre to
 * centre (a feature voxel reads 0).  border != 0: the one-voxel layer around the grid - the index -1 or G on any axis - counts as
 * features too (as the grid's border counts as unoccupied for the surface), so the inside distance of a full grid is finite:
 * min(i+1, Gx-i, j+1, Gy-j, k+1, Gz-k)^2.  A frame with an empty F and border == 0 reads SMIL_EDT_NONE everywhere.  g->origin and
 * g->voxel_size are not read.  workspace: smil_hull_edt_workspace_bytes(g) bytes of device memory (a second int32 grid when Gz, or Gy
 * of a slice of more than 65 536 cells, exceeds the 512 cells of a line the LDS path holds; 256 bytes otherwise).  Errors
 * (smil_last_error): a NULL g, occ, d2 or workspace; a grid extent < 1; (Gx+1)^2 + (Gy+1)^2 + (Gz+1)^2 >= 2^31 (the result must fit an
 * int32).  Every linear index is 64-bit: N Gx Gy Gz may exceed 2^31.
 * ---------------------------------------------------------------------------------------- */
#define SMIL_EDT_NONE 2147483647
size_t smil_hull_edt_workspace_bytes(const SmilHullGrid *g);
int smil_hull_edt(const SmilHullGrid *g, const uint8_t *occ, int32_t invert, int32_t border, int32_t *d2, void *workspace, void *stream);
/* The field at points (N,P,point_dim) float32, float64 arithmetic, every output rounded once to float32: value (N,P) and, unless
 * NULL, grad (N,P,point_dim), the exact derivative of value with respect to the point, in world units.  d2_out: a transform of the
 * hull; d2_in: NULL (an unsigned field) or the transform of its complement (a signed field, negative inside).
 * Per axis (origin, voxel: the frame's rows of g, HOST tables of 1 or N rows as for smil_hull_carve; G: the axis' extent):
 *   u = (p - origin) / voxel - 0.5     the continuous index: cell centres lie on the integers
 *   c = clamp(u, 0, G-1);  i0 = min(floor(c), G-2), or 0 when G == 1;  i1 = min(i0+1, G-1);  t = c - i0
 * A cell's value is r = sqrt((double)d2_out) - sqrt((double)d2_in) in voxels (no second term without d2_in); a d2_in equal to
 * SMIL_EDT_NONE counts as 0 and a cell whose d2_out is SMIL_EDT_NONE reads r = 0, so a frame without a hull gives value 0 and
 * gradient 0 inside the grid, not inf or NaN.
 *   value = voxel * ( trilinear(r; t) + |u - c|_2 ),   the interpolation (1-t) r[i0] + t r[i1] along x, then y, then z.
 * The second term is the distance from the point to the box of cell centres: it keeps the field continuous and pulls a point
 * outside the grid back towards it.  grad = the interpolation's slope (r[i1] - r[i0] along the axis, interpolated along the other
 * two; 0 on an axis whose u was clamped, u != c, and on an axis with G == 1) plus the unit vector (u - c) / |u - c| where that is
 * non-zero; the voxel size cancels.  At an integer u the rule for i0 - the cell to the right, except at the last - decides the
 * slope.  point_dim == 2: points are (y, x) pixels, the grid must have Gz == 1, y maps to axis j and x to axis i, there is no z, and
 * grad is (dy, dx).  A point with a non-finite coordinate gives value 0 and gradient 0.  workspace:
 * smil_hull_carve_workspace_bytes(g) bytes (the uploaded tables).  Errors: point_dim outside {2, 3}; point_dim == 2 with Gz != 1;
 * NULL d2_out, points, value or workspace; the grid and table checks of smil_hull_carve. */
int smil_field_sample(const SmilHullGrid *g, const int32_t *d2_out, const int32_t *d2_in, const float *points, int32_t point_dim, int64_t P,
                      float *value, float *grad, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * Hull meshes: a watertight, consistently oriented triangle mesh with vertex normals per frame of an occupancy grid - surface nets
 * on the lattice of voxel centres (smilify_amd/csrc/hull_mesh.hip).  An extension: the reference has no counterpart.  No gradient;
 * asynchronous on `stream`; ballots and gathers, no atomics: two calls give the same bits.  tests/hull_mesh_ref.py restates the rules.
 *
 * Samples.  Sample (i, j, k) is inside iff occ != 0; the lattice is padded by one layer of outside samples, index -1 and G on every
 * axis (the grid's border is unoccupied, as for the surface), which closes the mesh where a hull touches the grid.
 * Cubes.  Cube (i, j, k), every index in -1 .. G-1, spans samples i..i+1 x j..j+1 x k..k+1; its linear index is
 * (i+1) + (Gx+1)((j+1) + (Gy+1)(k+1)).  A cube is active iff its 8 corners are not all of one kind.
 * Vertices.  One per active cube, frames packed in order, ascending cube index within a frame.  The start position, in continuous
 * index coordinates (sample i at u = i), is the mean of the midpoints of the cube's sign-changing edges - edges enumerated by axis
 * a = x, y, z and, with u = (a+1) % 3, v = (a+2) % 3, corner offsets (u, v) = (0,0), (1,0), (0,1), (1,1); every summand is a multiple of
 * 0.5, so the sum is exact, and there is one division.  (Crossings interpolated from the signed distance field would be the same
 * midpoints: across a sign-changing lattice edge both squared distances are 1.  Hence occupancy is the only input.)
 * Faces.  Cube (i, j, k) owns the lattice edges from sample (i, j, k) along +x, +y, +z.  An owned edge along a whose samples differ in
 * kind emits the quad of the four cubes around it, cube offsets (du, dv) = (-1,-1), (0,-1), (0,0), (-1,0), in the reversed order
 * when the edge's lower sample is the outside one - (v1 - v0) x (v2 - v0) then points out of the hull - as the triangles (q0,q1,q2),
 * (q0,q2,q3).  Frames packed in order; within a frame ascending owner cube, then axis, then the two triangles.  Indices are
 * frame-local int64.
 * Relaxation.  weights (n_steps) HOST float64; step s moves every vertex by v += w_s (mean(neighbours) - v) and clamps it into its
 * own cube [i,i+1] x [j,j+1] x [k,k+1].  The neighbours of a cube are the cubes across those of its faces whose 4 samples are not all
 * of one kind, summed in the order -x, +x, -y, +y, -z, +z; a vertex without a neighbour stays.  Jacobi steps on float64 index
 * coordinates, no fused multiply-add.
 * Output.  verts = origin + (u + 0.5) * voxel_size per axis in float64 (three roundings, the frame's rows of the HOST tables as for
 * smil_hull_carve), rounded once to float32.  normals (or NULL): per vertex, over its cube's 12 edges in the order above, every
 * sign-changing edge names a quad; (v1 - v0) x (v2 - v0) of each of that quad's triangles that holds the vertex is added, on the
 * final float64 index coordinates scaled by voxel_size; the sum is normalised (a zero sum gives (0,0,0)) and rounded once to float32.
 *
 * Calls.  smil_hull_mesh_count fills vert_offsets and face_offsets (N+1) int64 - frame n owns rows offsets[n] .. offsets[n+1] of the
 * packed outputs, faces counted in triangles - and leaves masks and prefixes in the workspace (smil_hull_mesh_workspace_bytes(g)
 * bytes, 12 bytes per 64 cubes; the table SIZES of g lay it out, the tables are not read).  The caller reads the two totals, sizes
 * the outputs and a scratch buffer of smil_hull_mesh_scratch_bytes(n_verts, n_steps) bytes (the float64 positions - two buffers when
 * n_steps > 0 - and 9 bytes per vertex; what a workspace sized before the count could only hold for the worst case of a vertex per
 * cube), and calls smil_hull_mesh_write with the SAME g, occ and workspace and n_verts = vert_offsets[N], n_faces =
 * face_offsets[N]: verts (n_verts,3) float32, normals (n_verts,3) float32 or NULL, faces (n_faces,3) int64.  Figures that are not
 * the workspace's own leave the outputs unwritten (no kernel turns them into an index); both 0: nothing is launched.
 * Errors (smil_last_error): the grid and table checks of smil_hull_carve; a NULL pointer; a non-finite weight; n_steps < 0; NULL
 * weights with n_steps > 0; negative counts; a frame of 2^31 or more cubes, (Gx+1)(Gy+1)(Gz+1) (its vertex count could reach
 * 2^31); more than 2^28 workgroups of 2 048 cubes in all.  N (Gx+1)(Gy+1)(Gz+1) may exceed 2^31: every global index is 64-bit.
 * ---------------------------------------------------------------------------------------- */
size_t smil_hull_mesh_workspace_bytes(const SmilHullGrid *g);
int smil_hull_mesh_count(const SmilHullGrid *g, const uint8_t *occ, int64_t *vert_offsets, int64_t *face_offsets, void *workspace,
                         void *stream);
size_t smil_hull_mesh_scratch_bytes(int64_t n_verts, int32_t n_steps);
int smil_hull_mesh_write(const SmilHullGrid *g, const uint8_t *occ, void *workspace, void *scratch, int64_t n_verts, int64_t n_faces,
                         const double *weights, int32_t n_steps, float *verts, float *normals, int64_t *faces, void *stream);

/* ------------------------------------------------------------------------------------------
 * Exact distances between point clouds and triangle meshes with gradients (smilify_amd/csrc/point_mesh.hip).  An extension: the
 * reference has no counterpart (pytorch3d names the operation loss.point_mesh_face_distance).  The distance is the true Euclidean
 * distance to the CLOSED triangle by its seven Voronoi regions; degenerate faces are legal (an edge of zero length acts as its end
 * point, a face of zero area as the nearest of its three segments, three equal vertices as a point); pytorch3d's min_triangle_area
 * rule is not reproduced.  A brute-force float32 search over ALL faces decides WHICH face (strict <, a float32 tie goes to the
 * smaller index whatever `splits`), its value is the same formula in float64 from the float32 inputs, rounded once.  No float
 * atomics: two calls give the same bits.  tests/point_mesh_ref.py restates the rules.
 *
 * Inputs of all three: N meshes packed - verts (n_verts,3), faces (F_total,3) int32 into the packed verts, face_off (N+1) int32 the
 * first face of every mesh, max_faces the most faces of one mesh - and a padded cloud points (N,P,3) with lengths (N) int32 or NULL
 * (every cloud has P points).  A coordinate that is NaN, inf or above 3e38 in magnitude is not usable: a face with such a vertex, or
 * with a vertex index outside [0, n_verts), never wins, and such a point is treated as a non-finite one, in every call.
 * face_off, max_faces (and vert_off, max_verts) are the caller's statement about the meshes and are trusted: they size the launches,
 * and a max_faces / max_verts below a mesh's true count leaves that mesh's last rows of the outputs unwritten, without an error.
 * splits: over how many workgroups the candidates of one query are divided, 0 = chosen from the sizes.
 * workspace: smil_point_mesh_workspace_bytes(N, F_total, P, n_verts) bytes (0: bad sizes), one layout for the four calls.
 *
 * smil_point_face_distance: for every point the nearest face of its mesh: dist2 (N,P), face (N,P) int32 within the mesh, bary (N,P,3)
 * of the closest point (b >= 0, sum 1).  A non-finite point, a point at or beyond its cloud's length and a mesh in which no face
 * can win give +inf, -1 and 0.
 * smil_face_point_distance: for every face the nearest point of its mesh's cloud: dist2 (F_total), point (F_total) int32 within the
 * cloud, bary (F_total,3) of the closest point ON THE FACE.  A cloud of length 0 (or without a finite point) gives +inf, -1 and 0.
 * smil_point_mesh_backward: the gradient of sum_r g_r dist2_r over the records of one direction (by_face 0: idx = face (N,P) and g
 * (N,P); 1: idx = point (F_total) and g (F_total)).  With c the closest point of the recorded pair, recomputed in float64, and
 * e = p - c: d_points += 2 g e, d_verts[v_k] += -2 g b_k e (c minimises over the triangle; at a region boundary the selected
 * region's one-sided value).  Records with idx -1, out of range, or naming a point or face with an unusable coordinate add
 * nothing.  The barycentrics of the forward are not an input: they are outputs for the caller's use only.  d_points (N,P,3) and d_verts (n_verts,3) are
 * written in full.  vert_off (N+1) int32: the first vertex of every mesh; max_verts: the most vertices of one mesh.  Shared sums
 * are int64 fixed point with a unit that follows the mesh's largest addend: scaling every input by a power of two scales the
 * gradients exactly, and a permutation of the points leaves d_verts bit-identical.
 *
 * smil_point_mesh_winding: the generalised winding number winding (N,P) of every point with respect to its mesh: the sum over ALL
 * faces of the signed solid angle Omega / (4 pi) the face subtends at the point.  1 inside a closed mesh whose faces are oriented
 * outwards, 0 outside, -1 inside one oriented inwards, k inside k nested shells; on a mesh with holes or self-intersections a
 * smooth function that stays near those integers away from the defects (tests/winding_ref.py restates the rules).  Per pair, in
 * float32 in the mesh's power-of-two frame, with a = v0 - p, b = a + e1, c = a + e2 (e1 = v1 - v0, e2 = v2 - v0):
 *   det = a . (e1 x e2),  den = |a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|,  Omega / 2 = atan2(det, den).
 * A pair with det == 0 (either sign of zero) adds exactly 0: a degenerate face, a point in a face's plane, a point on a vertex; the
 * result never hangs on the sign of a zero.  A face that is not usable (above) adds 0.  A point with an unusable coordinate, or at
 * or beyond its cloud's length, gets NaN.  A mesh without faces gives 0.  Every pair's Omega / (4 pi) (|.| <= 0.5) is converted to
 * int64 fixed point with the unit 2^-(61 - bits(F_n)) and summed as an integer, the splits merged with integer atomics and the sum
 * converted once to float32: two calls, every `splits`, every order of the faces and a scaling of all inputs by a power of two
 * give the same bits.  Errors as smil_point_face_distance.
 * ---------------------------------------------------------------------------------------- */
size_t smil_point_mesh_workspace_bytes(int32_t N, int32_t F_total, int32_t P, int32_t n_verts);
int smil_point_face_distance(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N,
                             int32_t F_total, int32_t max_faces, const float *points, int32_t P, const int32_t *lengths, int32_t splits,
                             float *dist2, int32_t *face, float *bary, void *workspace, void *stream);
int smil_face_point_distance(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N,
                             int32_t F_total, int32_t max_faces, const float *points, int32_t P, const int32_t *lengths, int32_t splits,
                             float *dist2, int32_t *point, float *bary, void *workspace, void *stream);
int smil_point_mesh_backward(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, const int32_t *vert_off,
                             int32_t N, int32_t F_total, int32_t max_faces, int32_t max_verts, const float *points, int32_t P,
                             const int32_t *lengths, int32_t by_face, const int32_t *idx, const float *g, float *d_points,
                             float *d_verts, void *workspace, void *stream);
int smil_point_mesh_winding(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N,
                            int32_t F_total, int32_t max_faces, const float *points, int32_t P, const int32_t *lengths, int32_t splits,
                            float *winding /* (N,P) */, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * A bounding-volume hierarchy over the faces of packed meshes (smilify_amd/csrc/mesh_bvh.hip): the answers of
 * smil_point_face_distance - the same winner, bit for bit, the same float64 finish, the same outputs and rules for padded or
 * non-finite points and for meshes without a usable face - without the scan over all faces.  An extension.  Built once for meshes
 * that do not change, refitted when only their vertices move.  tests/mesh_bvh_ref.py restates the rules.
 *
 * The tree of mesh n is implicit: its faces stand in Morton order of their centroids (order (F_total) int32: sorted position ->
 * face within the mesh, the positions of mesh n at face_off[n] ..), SMIL_BVH_LEAF consecutive sorted faces are a leaf, the
 * L = ceil(F_n / SMIL_BVH_LEAF) leaves are padded to Lp, the next power of two (>= 1), and the nodes are numbered as a heap: root 1,
 * children of i: 2 i and 2 i + 1, leaf k: Lp + k.  Node i of mesh n is row 4 (face_off[n] / SMIL_BVH_LEAF + n) + i of boxes
 * (smil_bvh_nodes(N, F_total) rows of 6 floats: lo xyz, hi xyz; 0: bad sizes).  A box is the exact float32 minimum and maximum of
 * the vertices of the usable faces below it (usable as in the block above: indices inside [0, n_verts), finite coordinates); with
 * none it is empty (lo = +inf, hi = -inf) and never entered.  No pointers, no atomics in the tree: two builds give the same bits.
 * workspace: smil_bvh_workspace_bytes(N, F_total, P, n_verts) bytes (0: bad sizes; P = 1 for the calls without points).
 *
 * smil_bvh_codes: keys (F_total) int64 = mesh << 32 | the 30-bit Morton code of the face's centroid inside its mesh's bounding box,
 * SMIL_BVH_SENTINEL for a face that is not usable.  The caller sorts the keys with a STABLE sort (ties keep face order) and passes
 * the permutation perm (F_total) int64 (sorted position -> packed face) to
 * smil_bvh_build: writes order and boxes.  An entry of perm outside its mesh gives order -1: a row that never wins.
 * smil_bvh_refit: boxes once more from new vertices (same faces) in the stored order, without a sort.  Exactness never depends on
 * the quality of the order: a refitted tree answers exactly like a fresh one, only the number of faces visited differs.
 * smil_bvh_point_codes: keys (N,P) int64: the Morton code of every point inside its mesh's root box (clamped), SMIL_BVH_SENTINEL for
 * a point at or beyond its cloud's length or with an unusable coordinate: for callers that present their queries in spatial order.
 * smil_bvh_point_face_distance: dist2 (N,P), face (N,P) int32, bary (N,P,3) as smil_point_face_distance writes them.  One lane per
 * point, depth first, the nearer child first, the leaf's faces by the same float32 formula in the same power-of-two frame; the
 * running best is the key {bits of d^2, face} compared lexicographically, and a node is entered when the squared distance D^2 of the
 * point to its box satisfies D^2 <= (sqrt(best) + 2^-18)^2 (1 + 2^-19) in the frame (<=, never <: a float32 tie reaches the smaller
 * face index; 2^-18 covers the leaf formula's evaluation error).  evaluated (N,P) int32 or NULL: the number
 * of leaf faces evaluated for every point (0 for a padded point).  order and boxes are trusted no further than memory safety: a
 * tree of other meshes gives wrong answers, never an access outside the arrays.  Errors as smil_point_face_distance.
 * ---------------------------------------------------------------------------------------- */
#define SMIL_BVH_LEAF 8
#define SMIL_BVH_SENTINEL 1073741824 /* 2^30: above every 30-bit code */
size_t smil_bvh_workspace_bytes(int32_t N, int32_t F_total, int32_t P, int32_t n_verts);
size_t smil_bvh_nodes(int32_t N, int32_t F_total);
int smil_bvh_codes(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N, int32_t F_total,
                   int32_t max_faces, int64_t *keys, void *workspace, void *stream);
int smil_bvh_build(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N, int32_t F_total,
                   int32_t max_faces, const int64_t *perm, int32_t *order, float *boxes, void *workspace, void *stream);
int smil_bvh_refit(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N, int32_t F_total,
                   int32_t max_faces, const int32_t *order, float *boxes, void *workspace, void *stream);
int smil_bvh_point_codes(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N,
                         int32_t F_total, int32_t max_faces, const float *boxes, const float *points, int32_t P,
                         const int32_t *lengths, int64_t *keys, void *workspace, void *stream);
int smil_bvh_point_face_distance(const float *verts, int32_t n_verts, const int32_t *faces, const int32_t *face_off, int32_t N,
                                 int32_t F_total, int32_t max_faces, const int32_t *order, const float *boxes, const float *points,
                                 int32_t P, const int32_t *lengths, float *dist2, int32_t *face, float *bary,
                                 int32_t *evaluated /* (N,P) or NULL */, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SMILFIT_H_ */
