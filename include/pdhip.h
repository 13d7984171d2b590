/* pdhip.h -- C ABI of libpdhip.so: the MI355X (gfx950) implementation of PointDreamer's
 * project -> inpaint -> unproject texturing path.
 *
 * The reference (YuQiao0303/PointDreamer) exposes no FFI for this path; the boundary is the set of
 * Python call signatures demo.colorize_one_mesh uses (demo.py:93-95, 107-110, 127-129, 150-151,
 * 172-177, 203).  Each entry point below names the reference function (file:line) it replaces.
 * The Python shims in pointdreamer_amd/ keep the reference's names and tensor contracts and route
 * every call here through ctypes.
 *
 * Conventions
 *   - every pointer is a BORROWED device pointer (HBM) owned by the caller, contiguous, row-major;
 *     "bool" tensors are uint8 (torch.bool layout); index tensors are int64 unless stated;
 *   - every call enqueues asynchronously on `stream` (a hipStream_t; NULL = default stream) and never
 *     synchronises, except the few calls documented as returning a host value;
 *   - return value: 0 = OK, negative = error (PDHIP_E_*); pdhip_last_error() gives a thread-local
 *     message.  Nothing throws across the ABI;
 *   - the library holds no global mutable state; scratch memory is passed in by the caller
 *     (workspace pointers) or lives in an opaque handle created by *_create and freed by *_destroy.
 *     The pdhip_debug_set_* tuning / test hooks are THREAD-LOCAL switches (they steer the calling thread's
 *     subsequent launches only), so concurrent callers never see each other's settings.
 *   - camera parameters: 16 float32 per view = R(9, row-major world->camera) t(3) fx fy A B,
 *     NDC = (fx*xc/-zc, fy*yc/-zc, (A*zc+B)/-zc); see DESIGN.md "Arithmetic contract".
 */
#ifndef PDHIP_H
#define PDHIP_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PDHIP_OK 0
#define PDHIP_E_ARG (-1)      /* invalid argument */
#define PDHIP_E_HIP (-2)      /* HIP runtime error (message has the hipError string) */
#define PDHIP_E_STATE (-3)    /* handle in wrong state (e.g. weights missing) */
#define PDHIP_E_NOMEM (-4)
#define PDHIP_E_UNKNOWN_NAME (-5)   /* pdhip_unet_load_tensor: not a tensor of this architecture (strict=False callers skip it) */

int pdhip_version(void);
int pdhip_lab_build(void);   /* 0 for a product build; > 0: that many translation units carry a wrong-result PD_LAB_* timing switch (csrc/common.h) -- tests refuse such a library */
const char* pdhip_last_error(void);
/* test hook: the carve log.  While it is on, every region that a workspace-taking entry or a size query of the calling thread carves
 * (csrc/common.h, Carve::take) is recorded as (base, offset, bytes); a size query records a null base.  Everything in a workspace outside
 * the recorded regions is alignment slack that no kernel may touch.  on != 0 / 0 switches it on / off; either clears the log; returns the
 * previous state.  Off by default, thread-local, host code only. */
int pdhip_debug_carve_log(int on);
/* copies out up to `capacity` recorded (base, offset, bytes) triples, 3 uint64 each, in the order they were carved, and returns how many
 * regions were carved since the log was switched on: more than the 256 the log keeps, or more than capacity, means that some are missing */
int pdhip_debug_carve_log_read(uint64_t* triples, int capacity);

/* ---- P1: ours_utils.get_rendered_hard_mask_and_face_idx_batch, transform + crop part
 *      (pointdreamer/ours_utils.py:93-141).  minmax_ws: 4*V uint32 scratch.
 *      uv_centers[V,2], uv_scales[V] are written only when rescale != 0. */
int pdhip_project_points(const float* cam_params, int V, const float* vertices, int Vn,
                         const float* points, int N, int rescale, double padding,
                         float* pos /*[V,Vn,4]*/, float* vertice_uvs /*[V,Vn,2]*/,
                         float* uv_centers, float* uv_scales,
                         float* point_uvs /*[V,N,2]*/, float* point_depths /*[V,N]*/,
                         uint32_t* minmax_ws, void* stream);

/* ---- P2: the nvdiffrast.rasterize call at ours_utils.py:142-147 (also extract_texture_map.py:57).
 *      zkey_ws: V*R*R uint64 scratch (z keys of the atomic path / face setups of the LDS-tiled path).  Outputs hard_masks[V,R,R] u8, face_idxs[V,R,R] i64 (-1 empty),
 *      depths[V,R,R] f32 (0 empty). */
int pdhip_raster_mesh(const float* pos /*[V,Vn,4]*/, int V, int Vn, const int32_t* faces /*[F,3]*/, int F,
                      int R, uint64_t* zkey_ws, uint8_t* hard_masks, int64_t* face_idxs, float* depths,
                      void* stream);
/* the same with an explicit workspace: pdhip_raster_mesh_ws_bytes(V, F, R) bytes keep meshes up to 65 536 faces on the LDS-tiled path
 * (with the historical V*R*R*8 bytes it is taken up to R*R/17 faces only: 15.4 k at R = 512) */
size_t pdhip_raster_mesh_ws_bytes(int V, int F, int R);
int pdhip_raster_mesh_ws(const float* pos, int V, int Vn, const int32_t* faces, int F, int R, uint64_t* zkey_ws, size_t ws_bytes,
                         uint8_t* hard_masks, int64_t* face_idxs, float* depths, void* stream);
/* tuning / test hook: 0 = automatic (LDS-tiled rasteriser up to 65 536 faces), 1 = force the global 64-bit atomicMin path;
 * both produce identical images.  Returns the previous value. */
int pdhip_debug_set_raster_path(int path);

/* ---- nvdiffrast contract pieces used by the UV-atlas producer (models/get3d/extract_texture_map.py:57-63) and by
 *      optimize_color (pointdreamer/ours_utils.py:1700-1705): barycentrics (u,v) of triangle vertices 0 and 1 at each covered
 *      pixel centre (rast[...,0:2]), and interpolate(attr, rast, tri) = u*a0 + v*a1 + (1-u-v)*a2 (zeros where empty). */
int pdhip_raster_barycentrics(const float* pos /*[V,Vn,4]*/, int V, int Vn, const int32_t* faces, int R,
                              const int64_t* face_idxs /*[V,R,R]*/, float* bary /*[V,R,R,2]*/, void* stream);
int pdhip_interpolate(const float* attr /*[Na,C]*/, int C, const int32_t* tri /*[F,3]*/, const int64_t* face_idxs,
                      const float* bary, long long pixels, float* out /*[pixels,C]*/, void* stream);

/* ---- Evaluation renderer, shading stage (utils/camera_utils.py:379-554 render_textured_mesh, :735-828 render_per_vertex_color_mesh): from
 *      face_idxs [V,R,R] / bary [V,R,R,2] (pdhip_raster_mesh_ws + pdhip_raster_barycentrics, rows as the rasteriser leaves them) to the
 *      finished views in one pass per pixel, no uv_map in HBM.  a = u*a0 + v*a1 + ((1-u)-v)*a2 over attr [Na,C] / tri [F,3] (the
 *      contract of pdhip_interpolate).  C = 2: a is a UV, wrapped (uv - floor(uv), the reference's `% 1`) and looked up bilinearly in
 *      atlas [A,A,3] f32 with x = u*A - 0.5, y = v*A - 0.5 clamped to [0, A-1] (grid_sample align_corners=False, padding_mode='border');
 *      atlas row 0 is v = 0, the orientation colorize_one_mesh returns (the PNG of save_textured_mesh is that flipped).  C = 3: a is the
 *      colour (per-vertex colours), atlas must be NULL.  Lighting (light_dirs [L,3], 1 <= L <= 16, with face_normals [F,3] and cam_params
 *      [V,16]; L = 0 and NULLs: none): n = the face normal, negated where n . R[2] < 0 (cam_params[6:9], the camera's back axis); colour =
 *      clip(sum_l a * clip(n . l, 0, 1), 0, 1) with |n . l| when double_side, then ** (1 / gamma) when gamma > 0 (0: none).
 *      images [V,3,R,R] f32 and rgba [V,R,R,4] u8 (either may be NULL) are flipped vertically (row 0 = top, camera_utils.py:553-554);
 *      rgba = rint(colour * 255) clamped to 0 .. 255, alpha 255 -- the input of the PNG writer.  Uncovered pixels (face index < 0, or a
 *      face / attribute index outside its table) are exactly 0 in both. */
int pdhip_shade_views(const int64_t* face_idxs /*[V,R,R]*/, const float* bary /*[V,R,R,2]*/, int V, int R, const float* attr /*[Na,C]*/,
                      int Na, int C, const int32_t* tri /*[F,3]*/, int F, const float* atlas /*[A,A,3] or NULL*/, int A,
                      const float* face_normals /*[F,3] or NULL*/, const float* cam_params /*[V,16] or NULL*/,
                      const float* light_dirs /*[L,3] or NULL*/, int L, int double_side, double gamma, float* images /*[V,3,R,R] or NULL*/,
                      uint8_t* rgba /*[V,R,R,4] or NULL*/, void* stream);

/* ---- The same shading stage for meshes with SEVERAL materials (render_textured_mesh, camera_utils.py:379-554: face_material_idx[face_idx]
 *      per pixel, then one grid_sample per material per view there; one pass per output pixel here -- no uv map, no albedo image and no
 *      per-material mask in HBM).  face_idxs / bary / V / R, lighting, clip, gamma, the vertical flip, images and rgba: exactly the
 *      contract of pdhip_shade_views (one __device__ tail serves both kernels).  Per covered pixel of face f: corner UVs
 *      uvs[face_uvs_idx[f][k]] (uvs [T,2] f32 with face_uvs_idx [F,3] i64, both or neither; an index of -1, or no table: that corner's
 *      UV is (0,0), :397, :427-428), uv = (u*a0 + v*a1) + ((1-u)-v)*a2 (the contract of pdhip_interpolate), m = face_material[f]
 *      (face_material [F] i32; NULL: material 0).  The material set is pdhip_sample_mesh's: texels (u8 RGB images one after the other,
 *      rows as their files store them, row 0 at the top, texel_bytes in all), mat_offset [M] i64, mat_wh [M,2] i32 = (W, H), mat_kd
 *      [M,3] f32, 1 <= M <= 255.  mat_wh[m] = (0,0): the colour is mat_kd[m] bit for bit.  Otherwise the lookup rule written down under
 *      pdhip_sample_mesh, operation for operation (csrc/texture_lookup.h, the one definition both kernels call): fr = uv - floor(uv),
 *      gx = fr_u*2 - 1, gy = -(fr_v*2 - 1), x = ((gx+1) W - 1)/2, y = ((gy+1) H - 1)/2 clamped to [0, W-1] x [0, H-1] (NaN -> 0), the
 *      blend top + fy (bot - top), top = t00 + fx (t01 - t00), over texels t/255.0f.  (A square image I looked up here is atlas = I
 *      flipped vertically / 255 looked up by pdhip_shade_views.)  material_idx [V,R,R] i32 (may be NULL): m per pixel, flipped like the
 *      images, -1 where uncovered.  Nothing outside a table is dereferenced: a face index outside [0, F), a uv index outside [-1, T), a
 *      material outside [0, M), or an image (mat_offset, mat_wh) that does not lie inside the texel_bytes leaves the pixel UNCOVERED --
 *      colour exactly 0, alpha 0, material -1.  Refused before any launch (PDHIP_E_ARG): V, R, F not positive or R > 16384, V > 65536;
 *      M outside 1 .. 255; uvs without face_uvs_idx or the reverse, T <= 0 with them; texels NULL with texel_bytes > 0; images and rgba
 *      both NULL; L outside 0 .. 16, lights without normals and cameras, gamma without lights.  Does not synchronise.
 *      Measured: profiles/render_materials_bench.txt. */
int pdhip_shade_views_materials(const int64_t* face_idxs /*[V,R,R]*/, const float* bary /*[V,R,R,2]*/, int V, int R,
                                const float* uvs /*[T,2] or NULL*/, int T, const int64_t* face_uvs_idx /*[F,3] or NULL*/,
                                const int32_t* face_material /*[F] or NULL: material 0*/, int F,
                                const uint8_t* texels /*[texel_bytes] or NULL*/, int64_t texel_bytes, const int64_t* mat_offset /*[M]*/,
                                const int32_t* mat_wh /*[M,2]*/, const float* mat_kd /*[M,3]*/, int M,
                                const float* face_normals /*[F,3] or NULL*/, const float* cam_params /*[V,16] or NULL*/,
                                const float* light_dirs /*[L,3] or NULL*/, int L, int double_side, double gamma,
                                float* images /*[V,3,R,R] or NULL*/, uint8_t* rgba /*[V,R,R,4] or NULL*/,
                                int32_t* material_idx /*[V,R,R] or NULL*/, void* stream);

/* ---- Image metrics of the evaluation (utils/metric_utils/psnr_ssmi.py:44-147): a, b [N,H,W,C] u8 (C <= 4) -> per image sse [N] u64, the
 *      exact sum of squared differences (PSNR = 10 log10(255^2 H W C / sse) is left to the host), and ssim [N] f64, the mean SSIM with
 *      C1 = (0.01*255)^2, C2 = (0.03*255)^2 (either may be NULL).  gaussian = 0: skimage.metrics.structural_similarity(data_range=255,
 *      channel_axis=2) -- 7x7 uniform window, sample covariance (49/48), mean over the windows inside the image (skimage's 3-pixel crop),
 *      the window sums kept as integers up to the division.  gaussian = 1: psnr_ssmi.py:127-147 -- outer product of the 11-tap Gaussian of
 *      sigma 1.5 normalised to sum 1, "valid" region, population covariance, mean over pixels and channels.  LDS tiles with halo, separable
 *      filter, fixed-order reduction in two launches, no floating-point atomics: two calls give equal bits.  An image smaller than the
 *      window when ssim is asked for: PDHIP_E_ARG.  ws: pdhip_image_metrics_workspace_bytes(N, H, W) bytes.  Does not synchronise. */
size_t pdhip_image_metrics_workspace_bytes(int N, int H, int W);
int pdhip_image_metrics(const uint8_t* a, const uint8_t* b, int N, int H, int W, int C, int gaussian, uint64_t* sse /*[N] or NULL*/,
                        double* ssim /*[N] or NULL*/, void* ws, void* stream);

/* ---- UV unwrapping (the xatlas.parametrize call of xatlas_uvmap_w_face_id, models/get3d/extract_texture_map.py:42-44; the layout is
 *      this library's own): charts of faces sharing a dominant signed normal axis (n.axis >= cos 70 for every face of a chart),
 *      orthographic projection per chart, one world-to-texel scale for all charts, shelf packing with `gutter` texels around every
 *      chart, no texel centre covered twice (the rasteriser's coverage rules; overlapping charts are split and re-packed).
 *      vertices [Vn,3] f32, faces [F,3] i64 -> uvs [T,2] in [0,1] (capacity 3F entries: one per (chart, vertex) pair), tex_idx [F,3] i64,
 *      face_chart [F] i32 (chart id = the smallest face index of the chart), counts (device, 4 x i32): T, charts, split rounds,
 *      error flags.  ws: pdhip_uv_atlas_ws_bytes(Vn, F) bytes.  Synchronises `stream` once per packing round (one word read);
 *      a face index outside [0, Vn) or charts that cannot fit the atlas return PDHIP_E_ARG with the cause. */
size_t pdhip_uv_atlas_ws_bytes(int Vn, int F);
int pdhip_uv_atlas(const float* vertices /*[Vn,3]*/, int Vn, const int64_t* faces /*[F,3]*/, int F, int resolution, int gutter,
                   float* uvs /*[3F,2] capacity*/, int64_t* tex_idx /*[F,3]*/, int32_t* face_chart /*[F]*/,
                   int32_t* counts /*device: [0] = T uv entries used, [1] = charts, [2] = split rounds, [3] = error flags*/,
                   void* ws, void* stream);

/* ---- Surface reconstruction from the cloud (baselines/spr.py:recon_one_shape_SPR: normals for a point set + screened Poisson through
 *      pymeshlab on the CPU there; here a dense-grid Poisson solve and marching cubes on the device, the layout and the mesh are this
 *      library's own).  points [N,3] f32, N >= 16.
 *      pdhip_estimate_normals: k nearest neighbours (3 <= k <= 32, the point itself included) through a sorted cell list, normal =
 *      eigenvector of the smallest eigenvalue of the neighbourhood covariance, oriented (1) by the votes sign(n . (eye - p)) of the
 *      n_eyes (<= 64) Fibonacci eyes on the sphere of radius eye_radius * (largest extent) round the cloud's centre that SEE the point
 *      (pdhip_hidden_point_removal), (2) by up to 32 Jacobi rounds of the majority of sign(n_i . n_j) over the oriented neighbours,
 *      (3) by the nearest oriented neighbour.  counts (device, 4 x i32): points oriented by rule 1, 2, 3, and left as computed (no
 *      oriented neighbour); they add up to N.  ws: pdhip_estimate_normals_ws_bytes(N, k, n_eyes).
 *      pdhip_surface_recon: the indicator function chi (HIGHER INSIDE the solid; normals point outwards) on a grid of 2^depth cells per
 *      axis (depth 6, 7, 8; cell size h = largest extent / (0.75 * 2^depth), the cloud's bounding cube centred), solved by conjugate
 *      gradients to a relative residual of 1e-4, iso value = mean of chi at the points; marching cubes with one vertex per crossing grid
 *      edge: a closed, consistently oriented triangle mesh, counter-clockwise seen from outside, every component returned.
 *      vertices [vertex_capacity,3] f32, faces [face_capacity,3] i64 (never more than 3 (2^depth + 1)^3 vertices and 5 * 8^depth faces;
 *      a closed surface of area S has about 2 S / h^2 faces and half as many vertices); colors [N,3] / vertex_colors
 *      [vertex_capacity,3] (both or neither): colour of the nearest cloud point.  counts (device, 4 x i32): vertices, faces, solver
 *      iterations, 0; they are written even when the capacities are too small (PDHIP_E_ARG, nothing written past the buffers).
 *      info (device, 8 x f32): h, grid origin x y z, iso value, relative residual reached, splat radius, nodes per axis.
 *      Both synchronise `stream` (bounding box; solver status every 32 iterations; sizes).  Measured: profiles/surface_recon_bench.txt.  All points equal, points on a plane or a
 *      line, a solve that does not converge, an empty or inverted surface: PDHIP_E_ARG with the cause.  Two calls give equal bytes. */
size_t pdhip_estimate_normals_ws_bytes(int N, int k, int n_eyes);
int pdhip_estimate_normals(const float* points /*[N,3]*/, int N, int k, int n_eyes, double eye_radius, float* normals /*[N,3]*/,
                           int32_t* counts /*device [4]*/, void* ws, void* stream);
size_t pdhip_surface_recon_ws_bytes(int N, int depth);
int pdhip_surface_recon(const float* points /*[N,3]*/, const float* normals /*[N,3]*/, const float* colors /*[N,3] or NULL*/, int N, int depth,
                        float* vertices, int vertex_capacity, int64_t* faces, int face_capacity, float* vertex_colors /*or NULL*/,
                        int32_t* counts /*device [4]*/, float* info /*device [8]*/, void* ws, void* stream);
/* test hooks (csrc/surface_recon.hip; tests/test_gpu_spr_stages.py holds every stage to oracle/spr_stages.py through them).  Both entries above
 * carve every intermediate from the caller's workspace, and most of it is still there when they return; the two layout hooks say where: byte
 * offsets from `ws`, taken from the same carve functions on a base that is never dereferenced.  Host code only, no device work; PDHIP_E_ARG for a null pointer or for
 * sizes whose size query returns 0.
 * pdhip_debug_estimate_normals_layout: off [6] = cstart (i32, cells^3 + 1 used), spos ([N] float4: x, y, z in sorted order, w = the bits of the
 *   point's index), knn ([N,k] i32, original indices, row i = the neighbours of point i), eyes ([n_eyes,3] f64), vis ([n_eyes,N] u8),
 *   pdhip_estimate_normals_ws_bytes(N, k, n_eyes).
 * pdhip_debug_surface_recon_layout: off [8] = cstart, spos (as above, of the reconstruction's own cell list), snrm ([N] float4, sorted order: the
 *   normal times the sample weight, w = 0), chi ([M^3] f32, M = 2^depth + 1, x fastest: the solution), eflag ([M^3] u8: bit a set = the grid edge
 *   that leaves the node along axis a crosses the iso value), misc ([64] i32: vertices, faces, iterations, -, -, the bits of the iso value, the
 *   bits of the residual), f ([M^3] f32: OVERWRITTEN by the marching-cubes counts, hence the entry below), pdhip_surface_recon_ws_bytes(N, depth).
 * pdhip_debug_surface_recon_rhs: the front half of pdhip_surface_recon, through the same function -- box, grid, splat radius, cell list, sample
 *   weights, right-hand side -- then f -> f_out (device [M^3] f32).  info (device, 8 x f32): h, grid origin x y z, cell size and cells per axis of
 *   the cell list, splat radius, nodes per axis.  ws: pdhip_surface_recon_ws_bytes(N, depth); spos, cstart and snrm are left in it as the layout
 *   hook says.  Synchronises `stream`.  PDHIP_E_ARG before any device work: a null pointer, N outside 16 .. 2^24, depth outside 6 .. 8. */
int pdhip_debug_estimate_normals_layout(int N, int k, int n_eyes, uint64_t* off /*host [6]*/);
int pdhip_debug_surface_recon_layout(int N, int depth, uint64_t* off /*host [8]*/);
int pdhip_debug_surface_recon_rhs(const float* points /*[N,3]*/, const float* normals /*[N,3]*/, int N, int depth, float* f_out /*[M^3]*/,
                                  float* info /*device [8]*/, void* ws, void* stream);

/* ---- Mesh decimation to a target face count (baselines/spr.py:63-64 asks pymeshlab's meshing_decimation_quadric_edge_collapse(
 *      targetfacenum, preservetopology=True) on the CPU; here quadric-error edge collapses in rounds of mutually independent collapses
 *      on the device, csrc/simplify_mesh.hip -- the mesh is this library's own, not pymeshlab's).  Input: a CLOSED, CONSISTENTLY ORIENTED
 *      2-manifold (what pdhip_surface_recon emits), any number of components: every directed edge once, its reverse once, three different
 *      indices in [0, Vn) per face; anything else is refused (PDHIP_E_ARG, counts[3] = 2, no output written).  Per vertex one quadric
 *      (area-weighted plane quadrics of its faces, f64) carried through the collapses; per edge (u < v) the position minimising
 *      Q_u + Q_v (else the cheapest of u, v, midpoint), valid if u and v have exactly two common neighbours, at least three vertices
 *      surround the pair, and every remaining face round them keeps a positive area and turns by less than acos(0.2); per round the about
 *      (F - target) / 2 cheapest valid edges compete by a hashed unique key for their closed neighbourhoods, the winners collapse
 *      (v into u, colour of the endpoint nearer to the new position).  The topology is preserved (components, Euler characteristic of each,
 *      closed, oriented); faces and surviving vertices keep their input order; every output vertex is referenced.  Stops at
 *      F <= target_faces + 1 (F is even on a closed mesh), or when a round finds no collapse (flags bit 0, `stalled`: the mesh reached so
 *      far is returned, PDHIP_OK); more than 1024 rounds is PDHIP_E_ARG.  target_faces >= F: the mesh is copied through bit for bit,
 *      rounds = 0.  Synchronises `stream` (input check; one status read per 8 rounds).  Two calls give equal bytes.
 *      The size query returns 0 for Vn < 4, F < 4, Vn > 2^22 or F > 2^23 (the widths of the edge keys). */
size_t pdhip_simplify_mesh_workspace_bytes(int Vn, int F);
int pdhip_simplify_mesh(const float* vertices /*[Vn,3]*/, int Vn, const int64_t* faces /*[F,3]*/, int F, const float* vertex_colors /*[Vn,3] or NULL*/,
                        int target_faces, float* out_vertices /*[Vn,3]*/, int64_t* out_faces /*[F,3]*/, float* out_colors /*[Vn,3] or NULL*/,
                        int32_t* counts /*device [4]: vertices, faces, rounds, flags (1 = stalled, 2 = bad input)*/, void* ws, void* stream);

/* ---- Coloured clouds from textured meshes (data/sample_colored_pc_from_mesh.py:50-184: kal.ops.mesh.face_areas + sample_points and one
 *      grid_sample per material there), csrc/sample_mesh.hip.  A deterministic function of explicit uniforms rand [N,3] f32 in [0,1):
 *      kaolin's and torch's random streams are not reproduced.  vertices [Vn,3] f32, faces [F,3] i64, uvs [T,2] f32 with face_uvs_idx
 *      [F,3] i64 (both or neither; -1 at a corner = that corner's UV is (0,0), :102-107), face_material [F] i32 (NULL: material 0),
 *      face_keep [F] u8 (the reference's face_visibility; NULL: every face).  The material set of M materials: texels, u8 RGB images
 *      one after the other, each row-major as its file stores it (row 0 at the top), texel_bytes in all; material m's image starts at
 *      byte mat_offset[m] and is mat_wh[m] = (W, H) texels; mat_wh[m] = (0,0): no image, the colour is mat_kd[m] (mat_kd [M,3] f32).
 *      Face choice: A_f = 0.5 sqrt(|cross(v1-v0, v2-v0)|^2) in f64 (0 where face_keep is 0), Amax by an integer atomic max on the bit
 *      pattern, w_f = (uint64) floor(A_f * (2^40 / Amax)), cdf = inclusive uint64 prefix sum (the shared tiled scan), W = cdf[F-1];
 *      m = (uint32) floor(rand0 * 2^24) (held to [0, 2^24) whatever rand0 is), t = (W * m) >> 24 with the product exact in 128 bits, face =
 *      the smallest f with cdf[f] > t: exact integer arithmetic, so the choice does not depend on the scan order and a face of weight 0 is
 *      never drawn.  (u, v) = (rand1, rand2), folded to (1-u, 1-v) where u + v > 1 (kaolin); coords = (v0 + u (v1-v0)) + v (v2-v0) in f32
 *      op by op, uvs_out the same over the corner UVs, stored BEFORE the wrap (:179); normals = the unit face normal in f32
 *      (camera_utils.face_normals_unit, norm clamped at 1e-30); colors: mat_kd, or with fr = uv - floor(uv), gx = fr_u*2 - 1,
 *      gy = -(fr_v*2 - 1), x = ((gx+1) W - 1)/2, y = ((gy+1) H - 1)/2 clamped to [0, W-1] x [0, H-1] the bilinear blend
 *      top + fy (bot - top), top = t00 + fx (t01 - t00), over texels t/255.0f (:161-170: grid_sample align_corners=False,
 *      padding_mode='border').  Outputs coords, colors, normals [N,3] f32, uvs_out [N,2] f32, face_idx, material_idx [N] i32.
 *      face_idx ALWAYS indexes the caller's `faces`: the reference, given face_visibility, returns indices into the FILTERED face list
 *      next to normals of the unfiltered one (:110-113 against :173); that slip is not reproduced.
 *      An index outside its table is never dereferenced: a vertex index outside [0, Vn), a uv index outside [-1, T), a material index
 *      outside [0, M), an image outside the texel_bytes, a non-finite area -- the area pass skips the face and sets an error word; no
 *      face with positive area; F > 2^22 (refused before any launch): PDHIP_E_ARG with the cause, outputs untouched.  N = 0: the
 *      checks run, nothing is written, PDHIP_OK.  Synchronises `stream` ONCE (the error word and Amax, one read).  No floating-point
 *      atomics: two calls give equal bits.  ws: pdhip_sample_mesh_workspace_bytes(F, N) bytes (0 for F outside [1, 2^22]), carved by
 *      the one layout function both share.  Measured: profiles/sample_pc_bench.txt. */
size_t pdhip_sample_mesh_workspace_bytes(int F, int N);
int pdhip_sample_mesh(const float* vertices /*[Vn,3]*/, int Vn, const int64_t* faces /*[F,3]*/, int F, const float* uvs /*[T,2] or NULL*/, int T,
                      const int64_t* face_uvs_idx /*[F,3] or NULL*/, const int32_t* face_material /*[F] or NULL*/,
                      const uint8_t* face_keep /*[F] or NULL*/, const uint8_t* texels /*[texel_bytes] or NULL*/, int64_t texel_bytes,
                      const int64_t* mat_offset /*[M]*/, const int32_t* mat_wh /*[M,2]*/, const float* mat_kd /*[M,3]*/, int M,
                      const float* rand /*[N,3]*/, int N, float* coords /*[N,3]*/, float* colors /*[N,3]*/, float* normals /*[N,3]*/,
                      float* uvs_out /*[N,2]*/, int32_t* face_idx /*[N]*/, int32_t* material_idx /*[N]*/, void* ws, void* stream);

/* ---- SURVEY 8(e) configs[4], round 4: S independent shapes of EQUAL sizes (Vn vertices, F faces, N points, atlas A) through the same V
 *      cameras in ONE launch per stage.  Per-shape inputs are stacked ([S, ...]); every per-view array has S*V leading entries, view
 *      g = s * V + v; results equal the per-shape entry points bit for bit (tests/test_gpu_round4.py).  The per-view-independent stages
 *      (pdhip_resize_mask, pdhip_point_visibility*, pdhip_nearest_fill) already take any number of images: call them with S*V. */
int pdhip_project_points_shapes(const float* cam_params /*[V,16]*/, int V, int S, const float* vertices /*[S,Vn,3]*/, int Vn,
                                const float* points /*[S,N,3]*/, int N, int rescale, double padding, float* pos /*[S*V,Vn,4]*/,
                                float* vertice_uvs, float* uv_centers /*[S*V,2]*/, float* uv_scales /*[S*V]*/, float* point_uvs /*[S*V,N,2]*/,
                                float* point_depths /*[S*V,N]*/, uint32_t* minmax_ws /*[4*S*V]*/, void* stream);
int pdhip_raster_mesh_shapes(const float* pos /*[S*V,Vn,4]*/, int V, int S, int Vn, const int32_t* faces /*[S,F,3]*/, int F, int R,
                             uint64_t* zkey_ws, size_t ws_bytes /* pdhip_raster_mesh_ws_bytes(S*V, F, R) */, uint8_t* hard_masks,
                             int64_t* face_idxs, float* depths, void* stream);
int pdhip_hidden_point_removal_shapes(const float* points /*[S,N,3]*/, int N, const double* eyes /*[S*V,3]*/, int V, int S, double radius,
                                      const uint8_t* skip /*[S*V,N] or NULL*/, uint8_t* visibility /*[S*V,N]*/,
                                      void* ws /* pdhip_hpr_ws_bytes(S*V, N); S*V <= 64 */, void* stream);
int pdhip_sparse_views_shapes(const int64_t* point_pixels /*[S*V,N,2]*/, const float* colors /*[S,N,3]*/, const uint8_t* validation,
                              const uint8_t* hard_masks, int V, int S, int N, int res, int point_size, int edge_point_size,
                              double mask_ratio_thresh, float* sparse, float* mask0, float* mask2, float* scale_factors /*[S*V]*/,
                              float* mask_ratios, void* ws /* pdhip_sparse_views_ws_bytes(S*V, N, res) */, void* stream);
int pdhip_texel_visibility_shapes(const float* cam_params, int V, int S, const float* gb_pos /*[S,A,A,3]*/, const uint8_t* mask /*[S,A,A]*/,
                                  int A, const float* uv_centers, const float* uv_scales, double padding, const float* mesh_depths /*[S*V,R,R]*/,
                                  int R, float offset, uint8_t* visibility /*[S*V,A,A]*/, void* stream);
int pdhip_nbf_shrink_shapes(const uint8_t* mask /*[S,A,A]*/, const uint8_t* visibility /*[S*V,A,A]*/, int V, int S, int A,
                            const int32_t* kernels, int K, uint8_t* out /*[K][S*V][A][A]*/, uint8_t* ws /*2*S*V*A*A bytes*/, void* stream);
int pdhip_view_select_blend_shapes(const float* cam_params, int V, int S, const float* gb_pos, const uint8_t* mask, const int64_t* face_id,
                                   int A, const float* f_normals /*[S,F,3]*/, int F, const float* base_dirs /*[V,3]*/, const float* uv_centers,
                                   const float* uv_scales, double padding, const float* scale_factors, const uint8_t* shrinked /*[K][S*V][A][A]*/,
                                   int K, const uint8_t* visibility, int complete_unseen_by_projection, const float* inpainted /*[S*V,3,r,r]*/,
                                   int r, float* atlas /*[S,A,A,3]*/, uint8_t* painted /*[S,A,A]*/, int32_t* view_ids /*[S,A,A], local to the shape*/,
                                   void* stream);

/* ---- ours_utils.optimize_color (pointdreamer/ours_utils.py:1583-1785).
 *      pdhip_rescale_vertices: pos.xy <- clip((((xy-c)/s)*(1-2pad))*factor_v + 0.5, 0, 1)*2-1  (:1688-1695), in place.
 *      pdhip_optimize_color: `iterations` Adam steps (lr, StepLR(15, 0.5)) of the masked L1 texture loss, atlas[3,A,A] f32
 *      updated in place; uv_map[V,res,res,2] / face_idxs[V,res,res] are the UNflipped raster + interpolate outputs;
 *      shrinked[V,A,A] u8 may be NULL; final_images[V,3,res,res] f32 (render of the last iteration) may be NULL. */
int pdhip_rescale_vertices(float* pos /*[V,Vn,4]*/, int V, int Vn, const float* uv_centers, const float* uv_scales,
                           const float* factors /*[V]*/, double padding, void* stream);
size_t pdhip_optimize_color_ws_bytes(int V, int res, int A);
int pdhip_optimize_color(float* atlas, int A, const float* uv_map, const int64_t* face_idxs, int V, int res,
                         const float* inpainted /*[V,3,r,r]*/, int r, const uint8_t* shrinked, double lr, int iterations,
                         float* final_images, void* ws, void* stream);

/* ---- P2b: torchvision Resize(bilinear, no antialias) + .bool() on masks (demo.py:103-104,
 *      ours_utils.py:989-995): out is 1 iff any source pixel with non-zero bilinear weight is set. */
int pdhip_resize_mask(const uint8_t* in /*[B,in_h,in_w]*/, int B, int in_h, int in_w,
                      uint8_t* out /*[B,out_h,out_w]*/, int out_h, int out_w, void* stream);

/* ---- P3: ours_utils.get_point_validation_by_depth (ours_utils.py:153-202).
 *      point_pixels (row,col) may be NULL. */
int pdhip_point_visibility(int cam_res, const float* point_uvs /*[V,N,2]*/, const float* point_depths /*[V,N]*/,
                           const float* mesh_depths /*[V,R,R]*/, int V, int N, float offset,
                           uint8_t* visibility /*[V,N]*/, int64_t* point_pixels /*[V,N,2]*/, void* stream);

/* ---- P3b: ours_utils.get_point_validation_by_o3d (ours_utils.py:204-225), i.e. Open3D hidden_point_removal:
 *      spherical flip about each eye + convex-hull vertex test, all V views in one call, float64 on the device.
 *      eyes: V*3 float64 (device).  ws: pdhip_hpr_ws_bytes(V, N) bytes.  visibility[V,N] u8, written in full (it need
 *      not be cleared by the caller).
 *      skip (may be NULL): [V,N] u8; points already accepted by another test (demo.py:110 ORs the depth test with
 *      this one) are not queried and come back as 1, so the result is directly the OR-ed validation.
 *      Every verdict carries a floating-point certificate (separating direction / enclosing tetrahedron with error
 *      bounds) on the f64 coordinates; what the f64 certificates cannot decide is re-run as a distance iteration, first in
 *      f64, then in double-double arithmetic, so the result is the vertex set of the exact hull of the flipped points.
 *      pdhip_hpr_read_counters (synchronises) reports, for the last call on `ws`, summed over the views: out[0] queries
 *      sent to the double-double iteration, out[1] queries not certifiable even there (exactly degenerate input; reported
 *      hidden), out[2] double-double rounds, out[3] queries sent to the f64 distance iteration. */
size_t pdhip_hpr_ws_bytes(int V, int N);
int pdhip_hidden_point_removal(const float* points /*[N,3]*/, int N, const double* eyes /*[V,3]*/, int V, double radius,
                               const uint8_t* skip, uint8_t* visibility, void* ws, void* stream);
int pdhip_hpr_read_counters(const void* ws, int V, long long* out /*[4]*/, void* stream);

/* ---- demo.py:121-125: point_pixels = clip(long(uv*res)) as (row,col). */
int pdhip_point_pixels(const float* point_uvs /*[V,N,2]*/, int V, int N, int res,
                       int64_t* point_pixels /*[V,N,2]*/, void* stream);
/* both of the above in one pass over the points: the depth test at cam_res and the (row, col) pixels at res. */
int pdhip_point_visibility_pixels(int cam_res, const float* point_uvs, const float* point_depths, const float* mesh_depths,
                                  int V, int N, float offset, uint8_t* visibility /*[V,N]*/, int res,
                                  int64_t* point_pixels /*[V,N,2]*/, void* stream);

/* ---- P4-P6: ours_utils.get_sparse_images -> get_one_sparse_img -> paint_pixels /
 *      get_forground_inner_edge_mask (ours_utils.py:848-882, 954-1044, 456-532), all V views.
 *      ws: pdhip_sparse_views_ws_bytes(V,N,res) bytes.  Outputs are already flipped vertically and
 *      sparse is multiplied by mask0 (ours_utils.py:866).  Duplicate splats: largest write index wins. */
size_t pdhip_sparse_views_ws_bytes(int V, int N, int res);
int pdhip_sparse_views(const int64_t* point_pixels /*[V,N,2]*/, const float* colors /*[N,3]*/,
                       const uint8_t* validation /*[V,N]*/, const uint8_t* hard_masks /*[V,res,res]*/,
                       int V, int N, int res, int point_size, int edge_point_size, double mask_ratio_thresh,
                       float* sparse /*[V,3,res,res]*/, float* mask0, float* mask2,
                       float* scale_factors /*[V]*/, float* mask_ratios /*[V] or NULL*/,
                       void* ws, void* stream);

/* ---- I0 / Uq5: ours_utils.naive_inpainting(method='nearest') (ours_utils.py:610-643) and
 *      unproject.dilate_atlas (unproject.py:480-504): every pixel takes the value of its
 *      Euclidean-nearest site; ties -> lexicographically smallest (row,col).
 *      img/out: B images; element (b,c,y,x) at b*batch_stride + c*chan_stride + (y*W+x)*pix_stride.
 *      mask: per image H*W; mask_is_f32 != 0 -> float (site iff != 0), else uint8.
 *      mask_batch_stride in elements.  ws: pdhip_nearest_fill_ws_ints(B,H,W) int32. */
size_t pdhip_nearest_fill_ws_ints(int B, int H, int W);
int pdhip_nearest_fill(const float* img, float* out, int B, int C, int H, int W,
                       int64_t batch_stride, int64_t chan_stride, int64_t pix_stride,
                       const void* mask, int mask_is_f32, int64_t mask_batch_stride,
                       int32_t* ws, void* stream);

/* ---- I0, texture_gen_method='linear': ours_utils.naive_inpainting(method='linear') (ours_utils.py:610-643), i.e.
 *      scipy.interpolate.griddata(method='linear'): Delaunay triangulation of the sites + barycentric interpolation, NaN outside
 *      the sites' convex hull.  Every unknown pixel finds its own Delaunay triangle (lifted lower-hull facet over the pixel) with
 *      exact integer predicates evaluated in float64; where co-circular sites admit several triangulations a valid one is used.
 *      img/out [B,C,H,W] f32 contiguous, mask per image H*W (f32: site iff != 0, else uint8), H, W <= 2048.
 *      ws: pdhip_linear_fill_ws_bytes(B,H,W).  tri (may be NULL): [B,H,W,3] int32, the triangle's site indices (row-major site
 *      order), -1 at sites, -2 outside the hull.  pdhip_linear_fill_unresolved (synchronises): queries that hit the round cap (0). */
size_t pdhip_linear_fill_ws_bytes(int B, int H, int W);
int pdhip_linear_fill(const float* img, float* out, int B, int C, int H, int W, const void* mask, int mask_is_f32,
                      int64_t mask_batch_stride, void* ws, int32_t* tri, void* stream);
int pdhip_linear_fill_unresolved(const void* ws, int B, int H, int W, int* out, void* stream);
int pdhip_debug_set_linear_local(int on);   /* tuning / test hook: 1 (default) = two local window passes (8x8 tiles with 20x20 windows, then 16x16 tiles with 48x48 windows), global scans only for what they cannot certify; 2 = the 48x48 pass only; 0 = global scans only */

/* test / lab hook: 1 = Uq1-Uq4 run their run-time-view-count kernels even at V = 8 (default 0: the view loop is unrolled at V = 8 and
 * the view selection skips the softmax exponentials where the selected view provably does not depend on them; same results bit for
 * bit, tests/test_gpu_round5.py).  Returns the previous value; thread-local. */
int pdhip_debug_set_unproject_generic(int on);

/* ---- Uq1+Uq2: unproject.unproject texel transform + depth visibility (unproject.py:219-284).
 *      visibility[V,A,A] u8 (0 outside the chart mask). */
int pdhip_texel_visibility(const float* cam_params, int V, const float* gb_pos /*[A,A,3]*/,
                           const uint8_t* mask /*[A,A]*/, int A, const float* uv_centers /*[V,2]*/,
                           const float* uv_scales /*[V]*/, double padding,
                           const float* mesh_depths /*[V,R,R]*/, int R, float offset,
                           uint8_t* visibility, void* stream);

/* ---- N1-N3: unproject.get_shrinked_per_view_per_pixel_visibility_torch (unproject.py:429-475),
 *      utils_2d.detect_edges_in_gray_by_scharr_torch_batch (:799-827), dilate_torch_batch (:833-845).
 *      kernels: K host ints (odd, or kernels[0]==0 -> NBF off: out = visibility).
 *      out[K,V,A,A] u8.  ws: 2*V*A*A bytes. */
int pdhip_nbf_shrink(const uint8_t* mask /*[A,A]*/, const uint8_t* visibility /*[V,A,A]*/, int V, int A,
                     const int32_t* kernels, int K, uint8_t* out, uint8_t* ws, void* stream);
/* The path pdhip_nbf_shrink / pdhip_nbf_shrink_shapes take for V views in all (S * V for the shapes entry): host only, no device work, and the
 * very function the launcher routes through.  BYTES: one byte per texel, any A, V, radius and alignment.  BITS_*: 64 texels per word --
 * A % 64 == 0, A <= 4096, V >= 2, every radius (k - 1) / 2 < 64, (32 + k - 1) * (A / 64) * 16 <= 65536 bytes of LDS, out 16-byte and ws
 * 8-byte aligned; PACK16 packs with 16-byte loads (mask and visibility 16-byte aligned), BALLOT byte by byte.  COPY: kernels[0] == 0.
 * align_mask: bits 0-3 = low 4 address bits of (mask | visibility), bits 4-7 = low 4 address bits of out, bits 8-10 = low 3 address bits of ws.
 * PDHIP_E_ARG: sizes not positive, an even kernel size, or a bit path forced where it is not eligible. */
#define PDHIP_NBF_BYTES 0
#define PDHIP_NBF_BITS_PACK16 1
#define PDHIP_NBF_BITS_BALLOT 2
#define PDHIP_NBF_COPY 3
int pdhip_nbf_path(int V, int A, const int32_t* kernels, int K, unsigned align_mask);
/* test hook: 0 (default) = automatic, 1 = the byte path, 2 = the bit path with the ballot packer; a forced bit path that is not eligible is
 * refused by the launcher (PDHIP_E_ARG), never launched.  Returns the previous value; thread-local. */
int pdhip_debug_set_nbf_path(int mode);
/* Bit-packed transport of boolean texel maps (no reference counterpart: the reference is single-GPU; SURVEY 8(e) prices the view-parallel
 * all-gather record with its visibility maps bit-packed): bit i of out word w = (in[64 w + i] != 0); n % 64 == 0; 16-byte aligned byte side. */
int pdhip_pack_bits(const uint8_t* in /*[n] 0 / non-0*/, long long n, uint64_t* out /*[n / 64]*/, void* stream);
int pdhip_unpack_bits(const uint64_t* in /*[n / 64]*/, long long n, uint8_t* out /*[n] 0 / 1*/, void* stream);
/* the reference's always-on debug triptychs `others/shrink_per_view_edge/{v}.png` (unproject.py:459-474): per view
 * [visibility + background edges (red) + view edges (blue) | view edge mask | border mask of `kernel`] with 10 white columns
 * between panels, rows reversed; out [V][A][3A+20][3] u8 (HWC), ws (2V+1)*A*A bytes. */
int pdhip_nbf_triptych(const uint8_t* mask, const uint8_t* visibility, int V, int A, int kernel, uint8_t* out, uint8_t* ws,
                       void* stream);

/* ---- Uq3+Uq4: view selection + colour gather (unproject.py:298-400).
 *      shrinked[K,V,A,A] (K = number of NBF levels actually consulted), visibility[V,A,A] raw.
 *      view_ids[A,A] int32: chosen view, -100 unseen, -1 outside the chart mask.
 *      atlas[A,A,3] f32, painted[A,A] u8. */
int pdhip_view_select_blend(const float* cam_params, int V, const float* gb_pos, const uint8_t* mask,
                            const int64_t* face_id /*[A,A]*/, int A, const float* f_normals /*[F,3]*/,
                            const float* base_dirs /*[V,3]*/, const float* uv_centers, const float* uv_scales,
                            double padding, const float* scale_factors /*[V]*/,
                            const uint8_t* shrinked, int K, const uint8_t* visibility,
                            int complete_unseen_by_projection,
                            const float* inpainted /*[V,3,r,r]*/, int r,
                            float* atlas, uint8_t* painted, int32_t* view_ids, void* stream);

/* ---- texel compaction in row-major order (unproject.py:223-233): points[P,3], coords[P,2] i64,
 *      optional gather of view_ids[A,A] -> point_view_ids[P] i64.  Writes P to *count_dev (int32).
 *      ws: (A+1) int32. */
int pdhip_compact_texels(const float* gb_pos, const uint8_t* mask, int A, const int32_t* view_ids,
                         float* points, int64_t* coords, int64_t* point_view_ids, int32_t* count_dev,
                         int32_t* ws, void* stream);

/* =============================== rows U1 + D1: guided-diffusion UNet + DDNM ===============================
 * Replaces models/DDNM/ddnm_inpainting.py:15-44 (Inpainter), guided_diffusion/diffusion.py:435-570
 * (get_model, simplified_ddnm_inpainting) and guided_diffusion/unet.py:396-664 (UNetModel, fp16 torso).
 * The handle owns the repacked weights and an activation arena sized for max_batch images. */
typedef struct pdhip_unet pdhip_unet;

/* script_util.create_model (script_util.py:130-185): channel_mult / attention_ds are the already-resolved
 * integer tuples (for 256x256: mult (1,1,2,2,4,4), attention_ds (8,16,32)). */
int pdhip_unet_create(int image_size, int model_channels, int num_res_blocks, const int* channel_mult, int n_mult,
                      const int* attention_ds, int n_att, int num_head_channels, int out_channels, int max_batch,
                      pdhip_unet** out);
void pdhip_unet_destroy(pdhip_unet* u);
long long pdhip_unet_arena_bytes(const pdhip_unet* u);
/* host-only (no GPU needed): the route of every conv of a batch-N forward of the network pdhip_unet_create would build from the same arguments, under
 * the debug hooks in force -- one line per conv in launch order: "<layer> <H>x<W> <Cin>-><Cout> <kernel> <splits / slabs / variant> gn=<GroupNorm
 * partial chunks per image> <folds taken, or ->" (kernels: halo rr ht sk igemm phase; folds: gn_skip two_source apply in_gn in_up res_up skip
 * parts<-producer[+producer]).  Returns the length of the table, or a negative error; buf (may be NULL) gets what fits, NUL-terminated. */
int pdhip_unet_route_table(int image_size, int model_channels, int num_res_blocks, const int* channel_mult, int n_mult, const int* attention_ds,
                           int n_att, int num_head_channels, int out_channels, int max_batch, int N, char* buf, int buf_len);
int pdhip_unet_num_tensors(const pdhip_unet* u);
/* model.load_state_dict (diffusion.py:453): one call per state-dict entry, reference key names, PyTorch layouts
 * (conv OIHW, linear [out,in]); data is a device pointer to float32 (is_f16 = 0) or float16 (1). */
int pdhip_unet_load_tensor(pdhip_unet* u, const char* name, const void* data, int is_f16, const int64_t* shape, int ndim,
                           void* stream);
int pdhip_unet_missing_tensors(const pdhip_unet* u, char* buf, int buf_len);
/* UNetModel.forward (unet.py:635-664): x[N,3,S,S] f32, t[N] f32 -> out[N,out_channels,S,S] f32.
 * A handle owns its activation arena and split-K workspace (ticket words + slabs): at most ONE forward / sampler call of a handle may
 * be in flight at a time (calls on one stream are ordered by the stream; two streams need two handles). */
int pdhip_unet_forward(pdhip_unet* u, const float* x, const float* t, int N, float* out, void* stream);
/* HIP-event timing of the dominant kernel (3x3 implicit-GEMM conv launches) on the launch stream.  enable: 0 off, 1 every
 * forward, k > 1 every k-th forward (an event record costs the stream a few us of pipeline bubble; 108 of them per forward). */
int pdhip_unet_profile(pdhip_unet* u, int enable);
int pdhip_unet_profile_read(pdhip_unet* u, double* total_ms, double* total_flops, long long* launches);
/* the same for the attention launches (QK^T + softmax + PV, 4 T^2 C flop per image) -- north_star's MFMA-utilisation evidence */
int pdhip_unet_profile_read_attention(pdhip_unet* u, double* total_ms, double* total_flops, long long* launches);

/* D1 schedule (diffusion.py:46-113, 770-812): 100 steps t = 990..0; host arrays (any may be NULL). coefs[100][6] =
 * sqrt(1-a_t), sqrt(a_t), sqrt(a_next), sigma_t, c1, c2. */
int pdhip_ddnm_schedule(float* at, float* at_next, int* t, int* t_next, float* coefs);
/* y = mask * (2*img - 1)   (diffusion.py:477-484). */
int pdhip_ddnm_prepare(const float* masked_imgs /*[N,3,HW]*/, const float* masks /*[N,HW]*/, float* y, int N, int HW, void* stream);
/* one fused update (diffusion.py:529-552), in place on x; eps NULL -> on-device Philox noise. */
int pdhip_ddnm_step(float* x, const float* et, int et_channels, const float* y, const float* mask, const float* eps,
                    uint64_t seed, int step, int N, int HW, void* stream);
/* simplified_ddnm_inpainting for N images at once (the reference loops views serially at batch 1):
 * masked_imgs[N,3,S,S] in [0,1], masks[N,S,S] (1 = keep), optional injected x_T[N,3,S,S] and eps_tape[n_steps,N,3,S,S];
 * out[N,3,S,S] in [0,1]. */
int pdhip_ddnm_sample(pdhip_unet* u, const float* masked_imgs, const float* masks, int N, const float* x_T,
                      const float* eps_tape, uint64_t seed, int n_steps, float* out, void* stream);
/* the same with an explicit noise key: image n draws the Philox stream of key first_image_key + n, so a view's noise does not
 * depend on its batch position, on the batch composition or on how views are sharded over ranks (the reference draws
 * independent torch.randn noise per view, diffusion.py:493,552).  pdhip_ddnm_sample == first_image_key 0. */
int pdhip_ddnm_sample_keyed(pdhip_unet* u, const float* masked_imgs, const float* masks, int N, const float* x_T,
                            const float* eps_tape, uint64_t seed, uint64_t first_image_key, int n_steps, float* out, void* stream);

/* stand-alone operators of the engine (NHWC f16); also the unit-test surface of the kernels */
/* tuning / test hook: force the conv K-step (32 or 64; 0 = automatic); returns the previous value */
int pdhip_debug_set_conv_bk(int bk);
int pdhip_debug_set_conv_tile(int geometry);    /* 2 = 128x128 tile / 4 waves, 4 = 256x128 / 8 waves, 8 = 256x256 / 8 waves (wave tile 128x64),
                                                 * 16 = 256x128 / 4 waves, 32 = halo-resident 3x3 kernel (512x128); 0 = automatic */
int pdhip_debug_set_conv_stages(int stages);   /* 2..4 LDS pipeline stages, 12 = 2 stages + hand-scheduled fragment loop; 0 = automatic */
int pdhip_debug_set_conv_splitk(void* ws, long long ws_floats, int splits); /* split-K workspace for pdhip_conv2d_nhwc_f16 + forced factor (0 = automatic) */
int pdhip_debug_set_conv_halo_strips(int mode); /* halo-resident 3x3 kernel on 256-wide images: 0 = automatic (column strips of 128), 1 = full-row tiles; returns the previous value */
int pdhip_pack_conv_weight_f16(const float* w_oihw, int Cout, int Cin, int taps, void* w_packed /*[Cout][taps*Cin] f16*/, void* stream);
int pdhip_conv2d_nhwc_f16(const void* x, const void* w_packed /*[Cout_pad][taps*Cin]*/, const float* bias, const void* residual,
                          void* y, int N, int H, int W, int Cin, int Cout, int Cout_pad, int taps, const void* zero_page,
                          void* stream);
int pdhip_groupnorm_nhwc_f16(const void* x, const float* gamma, const float* beta, const float* film /*[N][2C] or NULL*/, int N,
                             int H, int W, int C, int silu, int resample, void* y, float* stats_ws, float* ws,
                             long long ws_floats, void* stream);
/* y = conv3x3( silu( GroupNorm32(x) [* (1 + scale) + shift] ) ) (+ residual): the in_layers / out_layers chain of a ResBlock
 * (unet.py:183-252: normalization -> SiLU -> conv, FiLM scale-shift in between for out_layers) with the normalisation applied INSIDE
 * the halo-resident conv kernel while it stages its input tile -- no stand-alone GroupNorm pass over the tensor.
 * W in {32, 64, 128, 256}, H*W % 512 == 0, Cin % 32 == 0; ws: N*64 + N*64*ceil(H*W/256) + N*Cin*2 floats. */
int pdhip_gn_silu_conv3x3_nhwc_f16(const void* x, const float* gamma, const float* beta, const float* film /*[N][2Cin] or NULL*/,
                                   long long film_stride, const void* w_packed, const float* bias, const void* residual, void* y,
                                   int N, int H, int W, int Cin, int Cout, int Cout_pad, const void* zero_page, float* ws,
                                   long long ws_floats, void* stream);
int pdhip_debug_conv3x3_apply(const void* x, const float* table /*[N][Cin/8][16]*/, const void* w_packed, const float* bias, const void* residual,
                              void* y, int N, int H, int W, int Cin, int Cout, int Cout_pad, const void* zero_page, void* stream);   /* tuning hook */
int pdhip_debug_set_fold_skip(int on);   /* 1 (default): in the small-M layers a channel-changing ResBlock's skip 1x1 conv (unet.py:206-209, 255) is appended to conv2's K loop (k_conv_sk<10>: out = W2 im2col(h) + Wskip x + (b2 + bskip), one launch and one rounding); 0: its own launch + a residual read; returns the previous value */
int pdhip_debug_set_up_phase(int mode);   /* in_layers conv of an up-ResBlock, conv3x3(nearest_x2(h)) (unet.py:190-192, 236-242), as four 2x2 phase convs over the half-resolution h with the coinciding taps summed in the weights (4/9 of the MACs): 0 never / 1 (default) where it measured faster / 2 every eligible layer; returns the previous value */
/* phase weights of that form: w_packed [Cout_pad][9*Cin] f16 -> w_phase [4][Cout_pad][4*Cin] f16 (phase = 2 py + px of the output pixel, k = (2 ty + tx) Cin + c over the
 * 2x2 source window); each entry the f32 sum in (ky, kx) order of the taps that land on one source pixel, rounded once to f16 */
int pdhip_pack_conv_up2_phase_f16(const void* w_packed, int Cin, int Cout_pad, void* w_phase, void* stream);
/* y [N,2H,2W,Cout] = conv3x3(nearest_x2(x [N,H,W,Cin]), pad 1) + bias through the four phase convs.  Cin % 64 == 0, Cout % 8 == 0, Cout_pad % 128 == 0,
 * gn_part (may be NULL; written only when H*W % 256 == 0): GroupNorm octet partials [N][4*H*W/256][Cout/8][2] */
int pdhip_conv3x3_up2_phase_nhwc_f16(const void* x, const void* w_phase, const float* bias, void* y, int N, int H, int W, int Cin, int Cout,
                                     int Cout_pad, const void* zero_page, float* gn_part, void* stream);
/* the same layer on the 9-tap halo-resident kernel, which reads source pixel (y >> 1, x >> 1) (the route the phase conv replaces; only layers that
 * kernel takes unsplit) */
int pdhip_conv3x3_up2_halo_nhwc_f16(const void* x, const void* w_packed, const float* bias, void* y, int N, int H, int W, int Cin, int Cout,
                                    int Cout_pad, const void* zero_page, void* stream);
int pdhip_debug_set_fold_resample(int on);   /* 1 (default): the resampled x branch of up / down ResBlocks is folded into its consumers; 0: k_resample passes */
int pdhip_debug_set_fold_finalize(int max_batch);   /* largest UNet batch at which GroupNorm-apply reduces the conv epilogues' statistics partials itself (no k_gn_finalize_oct launch); default 8, 0 = never */
int pdhip_debug_set_fold_finalize_chunks(int chunks);   /* above that batch the in-kernel statistics are kept for tensors whose producers left at most this many chunks per image (default 16; 0 = batch rule only); returns the previous value */
int pdhip_debug_set_conv_sk(int mode, int tile, int splits);   /* small-M conv kernel (in-launch split-K combine): mode 0 never / 1 automatic / 2 every eligible layer; tile 0 auto, 1..4 = 128x128, 128x64, 64x64, 64x32; splits 0 auto */
int pdhip_debug_set_conv_sk_stages(int stages);   /* lab hook: LDS stage count of the small-M conv kernel (2, 3, 4 where the tile allows; 0 = default) */
int pdhip_debug_set_conv_sk_kgroups(int kg);   /* lab hook: K-groups (4-wave groups working on alternate K-steps of one tile) per workgroup of the small-M conv kernel: 1, 2, 4 (64-row tiles), 8 = loader-specialised (4 compute + 4 loader waves), 12 = loader-specialised with EIGHT loader waves (the 128-row tiles; the default of the 128x128 tile since round 5); 0 = default */
int pdhip_debug_set_attn(int nbuf, int vt_form, int qtiles);   /* lab hook, T >= 128 attention kernel: qtiles = 16-query tiles per wave, 1 (64 queries per workgroup) or 2 (128), 0 automatic; nbuf = LDS chunk buffers, 2 (K / V requested one chunk ahead), 3 (two ahead), 0 automatic; vt_form 1 = V transposed into the workspace by a separate pass and read plainly, 0 = V staged row-major and read with the LDS transpose read */
int pdhip_debug_set_conv_sk_order(int order);   /* lab hook: tile order of the small-M conv kernel inside an XCD's run: 0 automatic, 1 pixel tiles fastest (weight slices shared through L2), 2 n-tiles fastest */
/* h0 = silu(GroupNorm32(x)) AND sk = conv1x1(x) (C -> 256 channels) in ONE pass over x: the in_layers normalisation and the
 * skip_connection of a channel-changing ResBlock (unet.py:197-209, 236-256) both read the block input, which for the decoder blocks is a
 * channel concat [xa (Ca channels) | xb (C - Ca)] that is never materialised (unet.py:657-659; xb NULL: x = xa, Ca == C).  stats [N][32][2] =
 * (mean, rstd) of x per GroupNorm group, finished (pdhip_groupnorm_nhwc_f16's stats_ws).  C % 256 == 0, Ca % 64 == 0, H*W % 128 == 0;
 * w_packed [256][C] f16, bias [256] f32 or NULL; h0 [N,H,W,C], sk [N,H,W,256] f16. */
int pdhip_gn_silu_skip1x1_nhwc_f16(const void* xa, const void* xb, int Ca, int C, const float* stats, const float* gamma, const float* beta,
                                   const void* w_packed, const float* bias, void* h0, void* sk, int N, int H, int W, void* stream);
int pdhip_debug_set_gn_iters(int iters);   /* lab hook: pixels per thread of the GroupNorm-apply kernel (1 .. 32; 0 = default); returns the previous value */
int pdhip_debug_set_gn_skip_variant(int v);   /* lab hook of the one-pass GroupNorm + skip kernel: 1 (default; 0 is taken as 1) = activation chunk k + 1 requested at the top of iteration k, 64-pixel tiles where 128-pixel tiles would leave CUs idle (< 256 tiles), 2 = as 1 with 128-pixel tiles always; returns the previous value */
int pdhip_debug_set_fuse_skip(int mode, int min_tiles);   /* ResBlock GroupNorm-apply + skip 1x1 as one pass: mode 0 never / 1 (default) layers of at least min_tiles 128-pixel tiles (default 1024; <= 0 keeps the value) / 2 every eligible layer; returns the previous mode */
int pdhip_debug_set_fuse_gn(int on);   /* 1: the UNet uses the fused form wherever the halo kernel serves a conv; 0 (default, measured faster): stand-alone passes */
/* ---- complete_unseen_by='neighbor' (pointdreamer/unproject.py:93-196, demo.py:180-200).
 * These are the per-texel / per-vertex kernels; the mesh work (subdivision, per-vertex UVs, neighbour table, list of uncoloured
 * vertices) runs on the device as well, through the entries of csrc/neighbor_mesh.hip declared after them. */
/* flags[f] = 1 for every face f that owns a chart texel no view painted (demo.py:180-181). face_id [A*A] int64 (-1 = background). */
int pdhip_mark_unpainted_faces(const int64_t* face_id, const uint8_t* painted, int A, int F, uint8_t* flags /*[F]*/, void* stream);
/* texel (row, col) = long(clip(uv * A, 0, A-1))[(1, 0)], colours = atlas[texel], count = mask[texel] (unproject.py:130-139) */
int pdhip_vertex_texel_fetch(const float* vert_uvs /*[V,2]*/, int V, const float* atlas /*[A,A,3]*/, const uint8_t* mask /*[A,A]*/,
                             int A, int32_t* texel /*[V,2]*/, float* colors /*[V,3]*/, float* count /*[V]*/, void* stream);
/* one Jacobi round of unproject.py:160-166 over the `invalid` vertices (CSR neighbours, ascending); *colored = number of
 * invalid vertices that hold a colour afterwards (device int; the host drives the loop as the reference does) */
int pdhip_neighbor_diffuse_round(const int32_t* rowptr /*[V+1]*/, const int32_t* colidx, int V, const int32_t* invalid, int IV,
                                 float* colors, float* count, float* tmp /*[IV*4]*/, int* colored, void* stream);
/* atlas[texel[v]] = colors[v], mask[texel[v]] = 1 (unproject.py:187-188); several vertices on one texel: largest index wins */
int pdhip_scatter_vertex_colors(const int32_t* texel, const float* colors, int V, float* atlas, uint8_t* mask,
                                int32_t* owner_ws /*[A*A]*/, int A, void* stream);
/* ---- the mesh side of 'neighbor' (utils/mesh_utils.py:7-114, unproject.py:105-127, 145-155) on the device, bit-identical to the numpy forms in
 * pointdreamer_amd/mesh_utils.py.  Sizes are int32; every entry checks them.  counts: device int32; counts_host (may be NULL): the same
 * values on the host -- each entry with a counts_host reads its counts and error flags back once, at its end (it synchronises
 * `stream`), and that one read is handed on, so a caller that needs the sizes reads nothing itself.
 *      pdhip_subdivide_with_uv: one round of midpoint subdivision of the faces in face_index [K] (duplicates allowed; NULL with K = -1:
 *      all faces; K = 0: the input comes back unchanged).  Untouched faces first in their order, then four children per picked face in
 *      ascending face order: (v0 m01 m20) (m01 v1 m12) (m20 m12 v2) (m01 m12 m20).  New vertices follow the old ones, one per unique
 *      undirected edge of the picked faces, ordered by (larger endpoint, smaller endpoint), value (x[lo] + x[hi]) / 2 in float32; the
 *      same rule runs independently on the UV index space.  With T picked faces (T <= Tmax = min(K, F), or F for all faces) the
 *      outputs hold V + E <= V + 3T vertices, U + Euv <= U + 3T UVs and F + 3T faces; the caller provides V + 3 Tmax, U + 3 Tmax and
 *      F + 3 Tmax rows.  counts[4] = V', U', F', T.  ws: pdhip_subdivide_with_uv_ws_bytes(V, U, F, K) bytes (non-decreasing in K >= 0).
 *      F <= 2^27, V, U <= 2^29.  A face_index entry outside [0, F), or a picked face with an index outside [0, V) / [0, U):
 *      PDHIP_E_ARG with the cause (the outputs are then undefined, within their capacities). */
size_t pdhip_subdivide_with_uv_ws_bytes(int V, int U, int F, int K);
int pdhip_subdivide_with_uv(const float* vertices /*[V,3]*/, int V, const int64_t* faces /*[F,3]*/, int F, const float* uvs /*[U,2]*/, int U,
                            const int64_t* face_uv_idx /*[F,3]*/, const int64_t* face_index /*[K] or NULL*/, int K,
                            float* out_vertices, int64_t* out_faces, float* out_uvs, int64_t* out_face_uv_idx,
                            int32_t* counts /*device [4]*/, int32_t* counts_host /*[4] or NULL*/, void* ws, void* stream);
/* one UV per vertex (unproject.py:123-127): of the UVs a vertex is used with, the one with the largest UV index; zeros for a vertex
 * no face uses.  counts[1] (device) = corners skipped because an index lies outside [0, V) / [0, U).  Does not synchronise. */
size_t pdhip_vertex_uv_table_ws_bytes(int V, int F);
int pdhip_vertex_uv_table(int V, const int64_t* faces /*[F,3]*/, const int64_t* face_uv_idx /*[F,3]*/, int F, const float* uvs /*[U,2]*/,
                          int U, float* vert_uvs /*[V,2]*/, int32_t* counts /*device [1]*/, void* ws, void* stream);
/* unique undirected vertex neighbours as CSR: rowptr [V+1], colidx ascending per row (capacity 6F), self pairs dropped;
 * counts[1] = nnz.  F <= 2^28.  A vertex index outside [0, V): PDHIP_E_ARG. */
size_t pdhip_neighbour_csr_ws_bytes(int V, int F);
int pdhip_neighbour_csr(int V, const int64_t* faces /*[F,3]*/, int F, int32_t* rowptr /*[V+1]*/, int32_t* colidx /*[6F] capacity*/,
                        int32_t* counts /*device [1]*/, int32_t* counts_host /*[1] or NULL*/, void* ws, void* stream);
/* invalid = ascending list of the vertices with count[v] == 0 (capacity V), counts[1] = its length (unproject.py:145-147) */
size_t pdhip_compact_zero_count_ws_bytes(int V);
int pdhip_compact_zero_count(const float* count /*[V]*/, int V, int32_t* invalid /*[V] capacity*/, int32_t* counts /*device [1]*/,
                             int32_t* counts_host /*[1] or NULL*/, void* ws, void* stream);

/* ---- I/O edges in native code (host functions; no device work except pdhip_chw_f32_to_hwc_u8).
 * PLY (utils/other_utils.py:155-163): vertex element with x,y,z and red,green,blue, binary_little_endian or ascii. */
long long pdhip_io_ply_count(const char* path);                 /* number of vertices, -1 on error */
int pdhip_io_read_ply_xyzrgb(const char* path, float* xyz /*[n,3] host*/, uint8_t* rgb /*[n,3] host*/, long long n);
/* OBJ + MTL, byte-identical to savemeshtes2 (models/get3d/get3d_utils/utils_3d.py:27-64). Host arrays (coordinates as
 * double: `%f` of a float32 value is printed from its exact double). */
int pdhip_io_write_obj_mtl(const char* obj_path, const char* mtl_path, const char* texture_stem, const double* points, long long P,
                           const double* tcoords, long long T, const int64_t* faces, const int64_t* facetex, long long F);
/* untextured OBJ (`v` with 9 significant digits: float32 round trip; `f a b c`), written to a per-process temporary and renamed */
int pdhip_io_write_obj_plain(const char* obj_path, const float* points /*[P,3] host*/, long long P, const int64_t* faces /*[F,3] host*/, long long F);
/* 8-bit RGB / RGBA PNG (utils/utils_2d.py:351-399 save path); hwc: host [H,W,channels] */
int pdhip_io_write_png(const char* path, const uint8_t* hwc, int H, int W, int channels, int zlib_level);
/* device: out[h,w,c] = uint8(clip(img[c,h,w] * 255, 0, 255)) -- the conversion the reference does on the host before saving */
int pdhip_chw_f32_to_hwc_u8(const float* img, int C, int H, int W, uint8_t* out, void* stream);

/* Output head of the UNet on its own (models/DDNM/guided_diffusion/unet.py:613-617): GroupNorm(32) -> SiLU -> conv3x3 in
 * float32-equivalent arithmetic.  x: f16 NHWC [N,H,W,C] (C in {32,64,128,256}); w_oihw f32 [Cout][C][3][3], Cout 3 or 6;
 * y f32 NCHW [N,Cout,H,W]; ws: pdhip_unet_head_ws_floats() device floats. */
size_t pdhip_unet_head_ws_floats(int N, int H, int W, int C, int Cout);
int pdhip_unet_head_f32(const void* x, const float* gamma, const float* beta, const float* w_oihw, const float* bias,
                        int N, int H, int W, int C, int Cout, float* y_nchw, float* ws, long long ws_floats, void* stream);
/* Row-resident convolution of the UNet's 8^2 / 16^2 / 32^2 levels at small batch (csrc/nn_conv_rr.hip): 3x3 (taps 9) or 1x1 (taps 1) conv over
 * x = [x (Ca channels) | x2 (C - Ca), may be NULL] with the GroupNorm32 (+ FiLM) (+ SiLU) of the input applied while staging -- the pair
 * `GroupNorm32 -> [scale / shift] -> SiLU -> conv` of ResBlock.in_layers / out_layers (guided_diffusion/unet.py:185-260) as ONE launch; gn_mode 0 raw input,
 * 1 GroupNorm, 2 GroupNorm + SiLU; statistics from the producers' octet partials partA / partB ([N][chunks][channels / 8][2] = sum, sum of squares);
 * film rows (scale[C] | shift[C]) or NULL.  xs / xs2 (Cs channels, Cs1 in xs): the ResBlock's skip_connection 1x1 (unet.py:255) appended to the K loop,
 * raw input, or NULL.  wf: fragment-major weights from pdhip_conv_rr_pack_f16 (source: [Cout_pad][taps * C + Cs] as pdhip_pack_conv_weight_f16 lays them out).
 * ws: >= 4096 zeroed floats (tickets) + split-K slices; gn_part (may be NULL): octet partials of y, *gn_chunks chunks per image.  H == W in {8, 16, 32}. */
int pdhip_conv_rr_f16(const void* x, const void* x2, int C, int Ca, int gn_mode, const float* gamma, const float* beta, const float* film,
                      long long film_stride, const float* partA, int chunksA, const float* partB, int chunksB, const void* xs, const void* xs2, int Cs,
                      int Cs1, int taps, const void* wf, const float* bias, const void* residual, int res_up, void* y, int N, int H, int W, int Cout,
                      float* ws, long long ws_floats, float* gn_part, int* gn_chunks, void* stream);
long long pdhip_conv_rr_weight_halfs(int Cin, int taps, int Cs, int Cout);
int pdhip_conv_rr_pack_f16(const void* w_packed, int Cin, int taps, int Cs, int Cout, void* wf, void* stream);
/* host-only: the largest number of GroupNorm(32) groups one staged unit of cs channels (128 or 256, by tile variant) of a C-channel source touches -- what
 * the kernel's in-staging statistics compute per unit; *capacity (may be NULL) = the groups the variant's statistics tables serve.  A source is accepted
 * with gn_mode != 0 only where the first does not exceed the second; 0 = not a channel count the kernel's group arithmetic serves. */
int pdhip_conv_rr_gn_groups_max(int cs, int C, int* capacity);
/* host-only: the plan pdhip_conv_rr_f16 would launch under the debug hooks in force: plan[7] = variant, conv slabs, units per slab, skip slabs, units per
 * skip slab, pixel bands per image, channel tiles; returns the variant (0: not a layer for the row-resident kernel). */
int pdhip_conv_rr_plan(int N, int H, int W, int Cin, int Cout, int taps, int Cs, long long ws_floats, int want_gn, int* plan);
/* test helpers: octet partials of a tensor as a conv epilogue leaves them; the two-pass reference of the fused input transform (k_gn_apply with in-kernel statistics) */
int pdhip_gn_octet_partials_f16(const void* x, int N, int HW, int C, int chunks, float* part, void* stream);
int pdhip_gn_apply_parts_f16(const void* x, const void* x2, int Ca, int C, const float* partA, int chunksA, const float* partB, int chunksB, const float* gamma,
                             const float* beta, const float* film, long long film_stride, int N, int H, int W, int silu, void* y, void* stream);
/* unit-test surface of conv_plan / conv_launch (csrc/nn_gemm.hip): pdhip_conv2d_nhwc_f16 with every operand a conv of the engine can carry.  The layer is
 * planned under the debug hooks in force and launched as planned; nothing is routed here.  x2 / Cin1: second tensor of a never-materialised channel concat
 * (1x1 only, Cin1 channels in x); residual read at half resolution with nearest x2 when res_up; xs / xs2 (Cs channels, Cs1 in xs; Cs == 0: none): the
 * ResBlock's skip 1x1 appended to the K loop -- w_packed is then [Cout_pad][9 Cin + Cs] (the 3x3 rows of pdhip_pack_conv_weight_f16 followed by the 1x1 rows)
 * and bias the sum of both.  ws (may be NULL): >= 4096 zeroed floats (tickets) + the split-K partials.  gn_part (may be NULL): octet partials of y,
 * [N][chunks][Cout / 8][2]; gn_part_floats: the floats the caller keeps there.  *kernel = the plan's kernel (0 halo, 1 rr, 2 ht, 3 sk, 4 igemm, 5 phase),
 * *gn_chunks = chunks per image: the plan's when the call is refused, what the launcher left otherwise.  PDHIP_E_ARG and no launch when the planned kernel
 * does not take an operand that was passed (x2, res_up, xs; a residual next to xs) or when gn_part_floats < N * chunks * (Cout / 8) * 2 -- a negative
 * gn_part_floats next to a gn_part therefore only plans (host-only, no device needed). */
int pdhip_debug_conv_launch_nhwc_f16(const void* x, const void* x2, int Cin1, const void* w_packed, const float* bias, const void* residual, int res_up,
                                     const void* xs, const void* xs2, int Cs1, int Cs, void* y, int N, int H, int W, int Cin, int Cout, int Cout_pad, int taps,
                                     const void* zero_page, float* ws, long long ws_floats, float* gn_part, long long gn_part_floats, int* gn_chunks, int* kernel,
                                     void* stream);
/* GroupNorm(32) statistics [N][32][2] = (mean, rstd), eps 1e-5, from the octet partials of one tensor (partB NULL, Cb 0) or of the two tensors of a channel
 * concat [A (Ca channels, chunksA chunks per image) | B (Cb, chunksB)]: the k_gn_finalize_oct launch of the engine.  (Ca + Cb) / 32 a multiple of 8. */
int pdhip_gn_finalize_oct_f32(const float* partA, int Ca, int chunksA, const float* partB, int Cb, int chunksB, int N, int HW, float* stats, void* stream);
/* 3x3 conv of the UNet's 64^2 / 128^2 levels at small batch on 256-pixel x 64-channel halo tiles (csrc/nn_conv_ht.hip; nn.Conv2d(k=3, padding=1) of
 * ResBlock.in_layers / out_layers, guided_diffusion/unet.py:185-260): x [N,H,W,Cin] f16, w_packed [Cout_pad][9 * Cin] from pdhip_pack_conv_weight_f16 (Cout_pad % 64 == 0),
 * H == W in {32, 64, 128}; residual optional (res_up: read at half resolution); splitk_ws (may be NULL: K unsplit): >= 4096 + tiles * slabs * 16384 floats, the first 4096
 * zeroed once (self-resetting ticket counters) -- K is cut in 2 / 4 slabs combined inside the launch when the tiles leave half of the CUs idle; gn_part (may be NULL):
 * GroupNorm octet partials of y, *gn_chunks = H * W / 256 per image. */
int pdhip_conv_ht_f16(const void* x, const void* w_packed, const float* bias, const void* residual, int res_up, void* y, int N, int H, int W, int Cin, int Cout,
                      int Cout_pad, const void* zero_page, float* splitk_ws, long long splitk_ws_floats, float* gn_part, int* gn_chunks, void* stream);
int pdhip_conv_ht_plan(int N, int H, int W, int Cin, int Cout, int Cout_pad, long long splitk_ws_floats, int* routed, int* slabs);   /* host-only: would the engine's automatic routing (step 7 of conv_plan, csrc/nn_gemm.hip) send this 3x3 layer to the halo-tile kernel, and in how many K-slabs */
int pdhip_debug_set_conv_ht(int mode, int slabs);   /* 256 x 64 halo-tile conv: mode 0 never / 1 automatic (batch 1-4 of the 64^2, 128^2 levels) / 2 every eligible layer; slabs 0 automatic, 1 / 2 / 4 forced K-slabs; returns the previous mode */
int pdhip_debug_set_rr_gn(int max_width);   /* UNet engine: largest image width at which a conv routed to the row-resident kernel also applies the GroupNorm (+ FiLM) + SiLU in front of it (default 0 = never: no gain measured inside the forward; 8 / 16 / 32 = up to that width); returns the previous value */
int pdhip_debug_set_conv_rr(int mode, int variant, int slabs);   /* row-resident conv: mode 0 never / 1 automatic / 2 every eligible layer; variant 0 auto (1: 8^2, 2: 16^2 half image, 3: 32^2 bands, 5: 8^2 with 128-channel units, 6 / 7: 32^2 / 16^2 with 16-channel tiles, 8: 64^2 bands; 6 - 8 take raw input only); slabs 0 auto = K slices of the conv source; returns the previous mode */
int pdhip_attention_f16(const void* qkv /*[N,T,3C]*/, void* out /*[N,T,C]*/, int N, int T, int C, int head_dim,
                        void* vt_ws /*N*T*C halfs, non-NULL selects the 128-query MFMA kernel for T % 128 == 0, head_dim 64, N*heads % 8 == 0 (QKVAttentionLegacy, unet.py:341-373); the buffer is written only in the transposed-V lab form (pdhip_debug_set_attn); NULL: the 64-query kernel*/, void* stream);
/* out[i] = element i of the N(0,1) stream (seed, stream_id): Philox4x32-10 with counter {i / 4 lo, i / 4 hi, stream_id lo, stream_id hi} and key {seed lo, seed hi};
 * the four words c give u = (float(c) + 0.5) 2^-32 and (sqrt(-2 ln u0) cos 2 pi u1, .. sin 2 pi u1, sqrt(-2 ln u2) cos 2 pi u3, .. sin 2 pi u3).  The sampler draws
 * x_T from stream 0 and the noise of step k from stream k + 1: pdhip_ddnm_step(eps NULL, seed, step k) adds exactly pdhip_philox_normal(N 3 HW, seed, k + 1). */
int pdhip_philox_normal(float* out, long long n, uint64_t seed, uint64_t stream_id, void* stream);
/* ---- the f32 side ops of the UNet on their own (csrc/nn_misc.hip): unit-test surface, nothing the product calls.
 * y [N][R] = W [R][K] x [N][K] + b [R], silu_out != 0: SiLU on top -- the batched GEMV behind time_embed and every ResBlock's emb_layers (unet.py:199-205,
 * 472-476).  All f32, W and x 16-byte aligned, K <= 2048 (8 x rows are staged in 64 KiB of LDS); a larger K is PDHIP_E_ARG and nothing is launched. */
int pdhip_gemv_rows_f32(const float* W, const float* b, const float* x, float* y, int R, int K, int N, int silu_out, void* stream);
/* emb_silu [N][4 mc] = silu(time_embed(timestep_embedding(t, mc))) (nn.py:103-121, unet.py:472-476; the SiLU is the first layer of every emb_layers):
 * w0 [4 mc][mc], w2 [4 mc][4 mc], PyTorch Linear layouts; mc even, <= 512.  tmp: N * 5 mc floats, on return [N][mc] the raw embedding
 * (cos | sin halves) followed by [N][4 mc] the hidden layer silu(w0 temb + b0). */
int pdhip_timestep_mlp_f32(const float* t, int N, int mc, const float* w0, const float* b0, const float* w2, const float* b2, float* emb_silu,
                           float* tmp, void* stream);
/* Y [N,H,W,Cout] f16 NHWC = conv3x3(x.half(), pad 1) + bias of the UNet's first conv (unet.py:483): x f32 NCHW [N,3,H,W]; Wt [Cout_pad][32] f16 with
 * k = (ky * 3 + kx) * 3 + c and k >= 27 zero, rows >= Cout zero; im2col_ws: N * H * W * 32 halfs (the gathered patches, one 32-wide row per pixel);
 * Cout % 8 == 0, Cout_pad % 128 == 0 (the GEMM behind it is pdhip_conv2d_nhwc_f16 as a 1x1 over 32 channels).  No GroupNorm partials. */
int pdhip_conv_in_f16(const float* x_nchw, const void* Wt, const float* bias, void* Y, int N, int H, int W, int Cout, int Cout_pad, void* im2col_ws,
                      const void* zero_page, void* stream);
/* ---- the GroupNorm-apply pass and its neighbours on their own (csrc/nn_norm.hip): unit-test surface, nothing the product calls.
 * y = [SiLU]( GroupNorm32(x) [* (1 + scale) + shift] ), optionally 2x resampled (resample 0 none, 1 AvgPool2d(2) of the activated values, 2 nearest x2), f16 NHWC:
 * the engine's gn_apply with every operand it can carry.  x [N,H,W,C], or with x2 the never-materialised channel concat [x (Ca channels) | x2 (C - Ca)].
 * The statistics come as exactly one of: stats [N][32][2] = (mean, rstd) finished, or the producers' octet partials partA ([N][chunksA][Ca / 8][2]; one tensor:
 * [N][chunksA][C / 8][2]) and, with x2, partB ([N][chunksB][(C - Ca) / 8][2]), reduced inside the kernel (C % 256 == 0, C <= 2048, eps 1e-5).
 * film: rows (scale[C] | shift[C]) f32, row n at film + n * film_stride, or NULL; only with resample 0.  y_raw (may be NULL; resample 1 and a single source only):
 * AvgPool2d(2) of the raw x, [N,H/2,W/2,C] f16.  Anything else is PDHIP_E_ARG and nothing is launched. */
int pdhip_gn_apply_f16(const void* x, const void* x2, int Ca, int C, const float* stats, const float* partA, int chunksA, const float* partB, int chunksB,
                       const float* gamma, const float* beta, const float* film, long long film_stride, int N, int H, int W, int silu, int resample, void* y,
                       void* y_raw, void* stream);
/* table [N][C / 8][16] = (A0..A7, B0..B7) per channel octet with GroupNorm32 (+ FiLM) = A x + B: A = rstd gamma t1, B = (beta - mean rstd gamma) t1 + sh,
 * t1 = f16(1 + f16(scale)), sh = f16(shift) (1 and 0 without film) -- the input transform of the halo conv's APPLY form.  C % 32 == 0. */
int pdhip_gn_table_f32(const float* stats, const float* gamma, const float* beta, const float* film, long long film_stride, int N, int C, float* table, void* stream);
/* y = AvgPool2d(2)(x) (mode 1: f16 of the f32 sum of the four pixels, in row-major order, times 0.25; H, W even) or nearest x2 (mode 2) of x [N,H,W,C] f16 NHWC, C % 8 == 0 */
int pdhip_resample2x_nhwc_f16(const void* x, int N, int H, int W, int C, int mode, void* y, void* stream);
/* y [pixels][Ca + Cb] = [a [pixels][Ca] | b [pixels][Cb]] f16 (th.cat over channels, unet.py:661); Ca, Cb % 8 == 0 */
int pdhip_concat_channels_f16(const void* a, int Ca, const void* b, int Cb, long long pixels, void* y, void* stream);
/* Calibration only (no reference counterpart): a streaming device-to-device copy, 16 bytes per lane, `unroll` & 15 (1, 2, 4, 8; 0 = 4) loads in
 * flight per lane, `unroll` >> 4 the form (0 grid-stride sweep, 1 the same with nontemporal loads / stores, 2 one contiguous slab per workgroup), `blocks` workgroups of 256 threads (0 = 2048).  bench.py reports its rate (read + write bytes) as
 * roofline.calibration.copy16_gbs next to torch's copy_: the ceiling the HBM-bound GroupNorm passes are judged against. */
int pdhip_bench_copy16(const void* src, void* dst, long long bytes, int blocks, int unroll, void* stream);

/* ---- geometry scores of a reconstruction (csrc/cloud_metrics.hip; models/POCO/eval/src/eval.py: distance_p2p, get_threshold_percentage, eval_pointcloud).
 * pdhip_nearest_points: for every query the EXACT nearest target.  queries [Q,3], targets [M,3] f32 on the device; with the inputs widened to f64,
 * dx = qx - tx (dy, dz alike) and d2 = (dx*dx + dy*dy) + dz*dz op by op, d2[q] is the minimum over all M targets and idx[q] the SMALLEST target index
 * that attains it: both equal a brute-force f64 scan bit for bit, and two calls give equal bytes (no floating-point atomics).  counts (device [4]):
 * queries certified by the LDS phase, queries finished by the ring scan from global memory (or, far from every target or in crowded cells, by the staged
 * sweep of all targets behind it), grid cells per axis, 0.  The shipped path is the ring scan for every query (counts[0] == 0); the LDS phase, which stages the targets of a workgroup's cell box in chunks of pdhip_nearest_points_stage_chunk()
 * targets and leaves the ring scan the queries it cannot certify, runs under pdhip_debug_set_nearest_path(1) and gives the same bytes.  ws: pdhip_nearest_points_workspace_bytes(Q, M) device
 * bytes (0 for sizes the entry refuses).  PDHIP_E_ARG with the cause, and d2 / idx / counts untouched: a non-finite coordinate in either cloud,
 * M < 1 or > 2^26, Q < 0 or > 2^26, a null pointer.  Q == 0: PDHIP_OK, counts zeroed.  The read of the two bounding boxes and of the two non-finite counts
 * SYNCHRONISES the stream once (64 bytes); the grid is laid over the part of the targets' box that the queries' box meets.  (The size query is not called ..._ws_bytes: tests/test_ws_bytes_cpu.py fixes the set
 * of queries with that suffix.) */
size_t pdhip_nearest_points_workspace_bytes(int Q, int M);
int pdhip_nearest_points_stage_chunk(void);
int pdhip_nearest_points(const float* queries, int Q, const float* targets, int M, double* d2, int32_t* idx, int32_t* counts, void* ws, void* stream);
int pdhip_debug_set_nearest_path(int path);   /* 0 (default): the one-thread-per-query ring scan from global memory for every query, the faster form at 10^5 x 10^5 points (profiles/geometry_metrics_bench.txt); 1: the LDS phase first, then the ring scan for the queries it could not certify (same results); returns the previous value */
/* pdhip_cloud_metrics: the sums behind completeness / accuracy / Chamfer / normal consistency / F-score over the output of pdhip_nearest_points.
 * d2 [Q] f64, idx [Q] i32 (into the M targets), normals_src [Q,3] and normals_tgt [M,3] f32 or NULL, thresholds [T] f64 ASCENDING on the device
 * (not checked), T <= 4096.  sums (device [4]) = sum sqrt(d2), sum d2, sum |n_src . n_tgt[idx]| with both normals normalised in f64 (a zero or
 * non-finite normal, or an idx outside [0, M), contributes 0; 0 when either normals pointer is NULL), 0.  The f64 sums run over a fixed tree (a
 * function of Q alone): equal bits on repeats.  within (device [T] i64): within[j] = queries with sqrt(d2) <= thresholds[j], exact (integer histogram
 * + prefix sum).  ws: pdhip_cloud_metrics_workspace_bytes(T) device bytes.  Q == 0: zeros. */
size_t pdhip_cloud_metrics_workspace_bytes(int T);
int pdhip_cloud_metrics(const double* d2, const int32_t* idx, int Q, const float* normals_src, const float* normals_tgt, int M,
                        const double* thresholds, int T, double* sums, int64_t* within, void* ws, void* stream);

/* ---- point-in-mesh test and volumetric IoU (csrc/occupancy.hip; models/POCO/eval/src/utils/libmesh/inside_mesh.py: check_mesh_contains,
 * eval/src/common.py: compute_iou).
 * pdhip_mesh_contains: occ[q] = 1 when point q is contained in the mesh by the reference's definition.  vertices [Vn,3] f32, faces [F,3] i64, points
 * [Q,3] f32 on the device, all widened to f64.  With R = resolution (the reference's hash_resolution, 512), over the vertices that a face REFERENCES:
 * scale = (R - 1) / (max - min) per axis, translate = 0.5 - scale * min, x' = scale * x + translate (two roundings) for triangles and points alike.  A
 * point outside [0, R]^3 is not contained.  A triangle (t1, t2, t3) is a hit for a point p when, with A = [t1 - t3, t2 - t3] in xy, detA = A00 A11 -
 * A01 A10 != 0, y = p - t3, u = (A11 y0 - A01 y1) sign(detA), v = (-A10 y0 + A00 y1) sign(detA): 0 < u < |detA|, 0 < v < |detA|, 0 < u + v < |detA| (all
 * strict).  For a hit, n = cross(t3 - t1, t2 - t1), alpha = n0 (t1x - px) + n1 (t1y - py), depth = t1z |n2| + alpha sign(n2); it counts above when depth
 * >= pz |n2|, below when depth < pz |n2|, in neither when n2 == 0.  occ = (above odd) and (below odd).  The result equals the all-pairs evaluation of
 * these formulas in f64, op by op, bit for bit; it depends on the order of neither the points nor the faces, and two calls give equal bytes (integer
 * atomics only).  resolution enters the result through the rescale alone: the cull is a grid over the POINTS whose size follows Q.  counts (device
 * [4]): contained, points whose two parities disagree (the reference's "contains1 != contains2" warning; an open mesh), points outside the box, 0.
 * ws: pdhip_mesh_contains_workspace_bytes(Vn, F, Q, resolution) device bytes (0 for sizes the entry refuses).  PDHIP_E_ARG with the cause, and occ /
 * counts untouched: a null pointer (named), Vn < 1, F < 1 or > 2^22, Q < 0 or > 2^26, resolution < 2 or > 4096, a face index outside [0, Vn), a
 * non-finite referenced vertex or point, a mesh without extent on an axis (the reference divides by zero).  Q == 0: PDHIP_OK, counts zeroed, the mesh
 * still validated.  The read of the bounding box and of the counts of bad inputs SYNCHRONISES the stream once (64 bytes).  (The size query is not called
 * ..._ws_bytes: tests/test_ws_bytes_cpu.py fixes the set of queries with that suffix.) */
size_t pdhip_mesh_contains_workspace_bytes(int Vn, int F, int Q, int resolution);
int pdhip_mesh_contains(const float* vertices, int Vn, const int64_t* faces, int F, const float* points, int Q, int resolution, uint8_t* occ,
                        int32_t* counts, void* ws, void* stream);
int pdhip_debug_set_mesh_contains_slabs(int slabs);   /* 0 (default): the column slabs per triangle of the per-triangle pass (each a group of lanes of its own) follow F (64 for a mesh of few faces, whose triangles span many columns of the point grid; 1 from 16 384 faces on); 1 .. 64: that many (same results; profiles/occupancy_bench.txt); returns the previous value */
/* pdhip_occupancy_iou: out (device [2] i64) = #{a >= 1 and b >= 1}, #{a >= 1 or b >= 1} over two [Q] u8 arrays on the device: integer counts only.
 * Q == 0: zeros.  PDHIP_E_ARG: Q < 0 or > 2^26, a null pointer (named). */
int pdhip_occupancy_iou(const uint8_t* a, const uint8_t* b, int Q, int64_t* out, void* stream);

/* ---- point-to-mesh distance (csrc/mesh_distance.hip; models/POCO/eval/src/eval.py: distance_p2m, i.e. trimesh.proximity.closest_point).
 * pdhip_closest_on_mesh: for every point the closest point of the mesh's surface, its squared distance and the face.  vertices [Vn,3] f32, faces [F,3]
 * i64, points [Q,3] f32 on the device, all widened to f64; every operation below is one f64 operation (no FMA, / correctly rounded).  With
 * dot(u,v) = (u.x v.x + u.y v.y) + u.z v.z, the closest point x of triangle (a, b, c) to q is Ericson's region walk:
 *   ab = b - a, ac = c - a, bc = c - b;  d1 = dot(ab, q - a), d2 = dot(ac, q - a);  d3 = dot(ab, q - b), d4 = dot(ac, q - b);  d5 = dot(ab, q - c),
 *   d6 = dot(ac, q - c);  vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4, e43 = d4 - d3, e56 = d5 - d6;  the first case that holds:
 *   1. d1 <= 0 and d2 <= 0: a;   2. d3 >= 0 and d4 <= d3: b;   3. vc <= 0, d1 >= 0, d3 <= 0: a + (d1 / (d1 - d3)) ab;   4. d6 >= 0 and d5 <= d6: c;
 *   5. vb <= 0, d2 >= 0, d6 <= 0: a + (d2 / (d2 - d6)) ac;   6. va <= 0, e43 >= 0, e56 >= 0: b + (e43 / (e43 + e56)) bc;
 *   7. otherwise, den = 1 / ((va + vb) + vc): (a + ab (vb den)) + ac (vc den).
 * The face's value is dot(q - x, q - x).  A face whose normal ab x ac (each component a difference of two products) is exactly (0, 0, 0) contributes
 * nothing; a face whose value is NaN never wins.  d2[q] is the minimum over the remaining faces, face[q] the SMALLEST index that attains it, closest[q]
 * (f64 [Q,3], or NULL: not wanted) that face's x; a point for which no face has a value gets d2 = +inf, face = -1, closest = NaN.  A per-face value
 * depends on no other face, so the result equals the all-pairs evaluation bit for bit on every path, depends on the order of neither the points nor
 * (apart from the index that wins a tie) the faces, and two calls give equal bytes (no floating-point atomics).  counts (device [4]): queries
 * certified by the ring scan over the cell list of the small faces, queries finished by the staged scan of all faces, faces on the large list (scanned
 * by every query: faces that span more than two cells of the grid on an axis, and slivers), degenerate faces skipped; counts[0] + counts[1] == Q.
 * ws: pdhip_closest_on_mesh_workspace_bytes(Vn, F, Q) device bytes, a function of (F, Q) alone (0 for sizes the entry refuses).  PDHIP_E_ARG with the
 * cause, and d2 / face / closest / counts untouched: a null pointer (named), Vn < 1, F == 0 or every face degenerate ("degenerate"), F > 2^23
 * (pdhip_simplify_mesh's limit), Q < 0 or > 2^26 (pdhip_nearest_points' limit), a face index outside [0, Vn), a non-finite referenced vertex or point.
 * An unreferenced vertex, finite or not, changes nothing.  Q == 0: PDHIP_OK, counts zeroed, the mesh still validated.  The read of the bounding box
 * and of the counts of bad inputs SYNCHRONISES the stream once (96 bytes).  (The size query is not called ..._ws_bytes: tests/test_ws_bytes_cpu.py
 * fixes the set of queries with that suffix.) */
size_t pdhip_closest_on_mesh_workspace_bytes(int Vn, int F, int Q);
int pdhip_closest_on_mesh(const float* vertices, int Vn, const int64_t* faces, int F, const float* points, int Q, double* d2, int32_t* face,
                          double* closest, int32_t* counts, void* ws, void* stream);
int pdhip_debug_set_closest_on_mesh(int cells_per_axis, int path);   /* test hook; same results under every setting.  cells_per_axis 0 (default): the grid's cells per axis follow F (sqrt(F / 32), at most 96); 1 .. 96: that many.  path 0 (default); 1: every live face on the large list; 2: every query to the all-faces scan.  Returns 4 * (previous cells_per_axis) + previous path */

/* ---- farthest-point subsampling (csrc/subsample.hip; no reference counterpart: demo.py:371-374 refuses clouds above 30 000 points).
 * pdhip_fps: M of the N points, each the farthest from those picked before it.  points [N,3] f32 on the device, widened to f64;
 * d2(i, j) = (dx*dx + dy*dy) + dz*dz with dx = xi - xj, op by op (pdhip_nearest_points' convention).  idx[0] = start, min_d2[0] = +inf; after pick k every
 * unselected point i has mind[i] = min over the picks so far of d2(i, pick); pick k + 1 is the unselected point with the largest mind, of those the
 * SMALLEST original index, and min_d2[k + 1] is that value.  A selected point is never selected again, also when mind is 0 everywhere (duplicates).
 * So min_d2[1:] never increases, and the first m picks of a run with M picks are the run with m picks.  idx (device [M] i32), min_d2 (device [M] f64)
 * equal the brute-force scan bit for bit: a cell list over the points' box prunes by a lower bound that never exceeds a member's computed d2.  Two calls
 * give equal bytes (no floating-point atomics).  counts (device [4]): cells per axis of the grid, occupied cells, point updates performed over all
 * picks (the brute-force scan performs N * M; saturates at 2^31 - 1), 0.  The pick loop runs in ONE workgroup (no cooperative launch, no barrier
 * across workgroups).  ws: pdhip_fps_workspace_bytes(N, M) device bytes, a function of N alone (0 for sizes the entry refuses).  PDHIP_E_ARG with the cause, and idx / min_d2 /
 * counts untouched: a null pointer (named), N < 1 or > 2^24, M < 1 or > N, start outside [0, N), a non-finite coordinate.  The read of the bounding
 * box and of the non-finite count SYNCHRONISES the stream once (32 bytes).  (The size query is not called ..._ws_bytes: tests/test_ws_bytes_cpu.py
 * fixes the set of queries with that suffix.) */
size_t pdhip_fps_workspace_bytes(int N, int M);
int pdhip_fps(const float* points, int N, int M, int start, int32_t* idx, double* min_d2, int32_t* counts, void* ws, void* stream);
/* pdhip_owner_mean_colors: the mean colour of the points each sample owns (a box filter over the subsample's Voronoi cells).  owner [N] i32 in [0, M):
 * the position in the selection of the sample nearest to point i (pdhip_nearest_points(points, N, points[idx], M)); colors [N,3] f32 in [0, 1];
 * fallback, out [M,3] f32; all on the device.  Per sample and channel sum = sum of llrint(c * 2^32) (c widened to f64) over its points, an int64 built
 * with integer atomics, and their count; out = (f32)(((f64)sum / (f64)count) / 2^32).  A sample that owns nothing (a duplicate of an earlier sample)
 * takes fallback.  Exact, independent of the order of the points, equal bytes on repeats.  ws_or_null: pdhip_owner_mean_colors_workspace_bytes(M) device
 * bytes, or NULL: the entry allocates and frees its own, and synchronises once more.  PDHIP_E_ARG with the cause, and out untouched: a null pointer
 * (named), N < 0 or > 2^26, M < 1 or > 2^26, an owner outside [0, M), a colour outside [0, 1] or non-finite.  The read of the two counts of bad inputs
 * SYNCHRONISES the stream once (8 bytes). */
int pdhip_debug_set_fps_cells(int cells_per_axis);   /* tuning / test hook; same results under every setting.  0 (default): the grid's cells per axis follow N (cbrt(N / 32), at most 40); 1 .. 40: that many (1: every pick updates every point).  Returns the previous value */
size_t pdhip_owner_mean_colors_workspace_bytes(int M);
int pdhip_owner_mean_colors(const int32_t* owner, const float* colors, int N, int M, const float* fallback, float* out, void* ws_or_null, void* stream);

/* ---- exact k nearest neighbours and statistical outlier removal (csrc/knn.hip; no reference counterpart: `input_already_noisy` only picks a POCO
 * weight set there.  The filter is PCL's StatisticalOutlierRemoval / Open3D's remove_statistical_outlier).
 * pdhip_knn_points: for every query the EXACT k nearest targets.  queries [Q,3], targets [M,3] f32 on the device; with the inputs widened to f64,
 * dx = qx - tx (dy, dz alike) and d2 = (dx*dx + dy*dy) + dz*dz op by op, row q of d2 (device [Q,k] f64) and idx (device [Q,k] i32) holds the k SMALLEST
 * pairs (d2, target index) in ascending lexicographic order: equal distances are ordered by index, and the same order decides the set when the tie
 * falls at the k-th place.  Both equal a brute-force f64 scan followed by a stable sort bit for bit, do not depend on the order of the queries, and two
 * calls give equal bytes (no floating-point atomics); with k == 1 they are the bytes of pdhip_nearest_points.  k = 1 .. pdhip_knn_max_k() (64).
 * counts (device [4]): queries certified by the ring scan over the targets' cell list, queries finished by the staged sweep of all targets behind it
 * (far from every target, or in crowded cells), grid cells per axis, 0; counts[0] + counts[1] == Q.  Every thread keeps its candidate list in LDS:
 * pdhip_knn_lds_bytes(k) = 12 * 65 * k bytes per workgroup of 64 queries.  ws: pdhip_knn_points_workspace_bytes(Q, M, k) device bytes, a function
 * of (Q, M) alone (0 for sizes the entry refuses).  PDHIP_E_ARG with the cause, and d2 / idx / counts untouched: a null pointer (named), k < 1,
 * k > 64 or k > M, M < 1 or > 2^26, Q < 0 or > 2^26, a non-finite coordinate in either cloud.  Q == 0: PDHIP_OK, counts zeroed.  The read of the two
 * bounding boxes, of the two non-finite counts and of the targets' per-axis coordinate histograms SYNCHRONISES the stream once (64 bytes + 12 KiB);
 * the grid is laid over the part of the targets' span -- their box cut per axis to the 1 % .. 99 % quantiles and widened by a tenth, so that a few
 * far points do not decide the cell size -- that the queries' box meets.  (The size query is not called ..._ws_bytes: tests/test_ws_bytes_cpu.py fixes the set of queries with that suffix.) */
size_t pdhip_knn_points_workspace_bytes(int Q, int M, int k);
int pdhip_knn_max_k(void);
size_t pdhip_knn_lds_bytes(int k);
int pdhip_knn_points(const float* queries, int Q, const float* targets, int M, int k, double* d2, int32_t* idx, int32_t* counts, void* ws, void* stream);
int pdhip_debug_set_knn(int cells_per_axis, int path);   /* tuning / test hook; same results under every setting.  cells_per_axis 0 (default): the grid's cells per axis follow M and k (sqrt(M / max(8, k / 2)), at most 128); 1 .. 64: that many.  path 0 (default): the ring scan, then the sweep for the queries it gave up; 1: the sweep for every query; 2: as 0 with the grid over the targets' whole box (no quantile cut).  Returns 4 * (previous cells_per_axis) + previous path, or -1 (and changes nothing) for a value outside these ranges */
/* pdhip_sor_filter: statistical outlier removal over the output of pdhip_knn_points.  knn_d2 [N,kk] f64 on the device: the kk = k + 1 nearest neighbours
 * of every point of a cloud in the cloud itself; slot 0 (the point itself, or a duplicate of it with a smaller index: distance 0 either way) is skipped.
 * mean_d[i] = (sum over j = 1 .. k of sqrt(knn_d2[i][j])) / k, summed sequentially in slot order in f64; mu = mean of mean_d,
 * sigma = sqrt(sum (mean_d - mu)^2 / (N - 1)) in two passes, both sums over a fixed tree that is a function of N alone (equal bits on repeats);
 * t = mu + std_ratio * sigma; stats (device [4] f64) = mu, sigma, t, 0; keep[i] (device [N] u8) = mean_d[i] <= t; kept_idx[0 .. counts[0]) (device [N]
 * i32) = the kept indices, ascending; counts (device [4]) = kept, removed, 0, 0.  ws: pdhip_sor_filter_workspace_bytes(N) device bytes (0 for sizes
 * the entry refuses).  PDHIP_E_ARG with the cause, and nothing written: a null pointer (named), N < 2 or > 2^26, kk < 2 or > 64, std_ratio negative
 * or not finite, a negative or non-finite knn_d2.  The read of the count of bad distances SYNCHRONISES the stream once (4 bytes). */
size_t pdhip_sor_filter_workspace_bytes(int N);
int pdhip_sor_filter(const double* knn_d2, int N, int kk, double std_ratio, double* mean_d, double* stats, uint8_t* keep, int32_t* kept_idx,
                     int32_t* counts, void* ws, void* stream);

/* ---- connected components of a mesh and compaction to a subset of its faces (csrc/mesh_components.hip; no reference counterpart: the filter on top,
 * mesh_components.filter_components, is MeshLab's "Remove isolated pieces").
 * pdhip_mesh_components: faces [F,3] i64 on the device, ANY indexed triangle list with indices in [0, Vn): it need not be closed, manifold or oriented,
 * and a face may repeat an index.  Two vertices are connected when some face names both; a component is a class of the transitive closure over the
 * referenced vertices.  Its root is its smallest vertex index, and the components are numbered 0 .. C-1 by ascending root.  vertex_comp (device [Vn]
 * i32): the component of every vertex, -1 for a vertex no face names; face_comp (device [F] i32) = vertex_comp[faces[f][0]]; per component
 * comp_root, comp_vertices, comp_faces (device [comp_capacity] i32: smallest index, vertices, faces) and, when comp_box is not NULL (vertices [Vn,3]
 * f32 on the device are then required, and otherwise never read), comp_box (device [comp_capacity,6] f32: min x y z, then max x y z, over the
 * component's vertices).  counts (device [4]): C, referenced vertices, unreferenced vertices, 0.  The per-component arrays hold comp_capacity
 * entries: when C > comp_capacity the entry still writes vertex_comp, face_comp, counts and the entries of the first comp_capacity components and
 * returns PDHIP_OK -- the caller reads C and calls again (entries from C on are never written).  Every output is a function of the mesh alone:
 * it depends on neither the order of the faces, nor the rotation of a face's indices, nor the threads' order, and two calls give equal bytes
 * (a lock-free union-find that keeps parent[v] <= v, integer atomics, boxes by atomicMin / atomicMax on the ordered encoding of the f32 bits; a
 * box bound that is zero may carry either sign).  ws: pdhip_mesh_components_workspace_bytes(Vn, F) device bytes (0 for sizes the entry refuses).
 * PDHIP_E_ARG with the cause, and every output untouched: a null pointer (named; only vertices and comp_box may be NULL, comp_box without vertices
 * may not), Vn < 1, F < 0, Vn > 2^26, F > 2^23, comp_capacity < 0, a face index outside [0, Vn), a referenced vertex that is not finite when boxes
 * are asked for.  F == 0: PDHIP_OK, counts = 0, 0, Vn, 0, every vertex_comp -1, no synchronisation.  Otherwise the read of the check words and of C
 * SYNCHRONISES the stream once, after the last launch (32 bytes).  Every walk of the union-find goes to strictly smaller indices and is bounded by
 * 2 Vn + 64 steps all the same; should one use them up, PDHIP_E_STATE and no output.  (The size queries are not called ..._ws_bytes:
 * tests/test_ws_bytes_cpu.py fixes the set of queries with that suffix.) */
size_t pdhip_mesh_components_workspace_bytes(int Vn, int F);
int pdhip_mesh_components(const int64_t* faces, int F, const float* vertices_or_null, int Vn, int32_t* vertex_comp, int32_t* face_comp,
                          int32_t* comp_root, int32_t* comp_vertices, int32_t* comp_faces, float* comp_box_or_null, int comp_capacity,
                          int32_t* counts, void* ws, void* stream);
/* pdhip_compact_mesh: the faces with face_keep[f] != 0 (device [F] u8) and the vertices they name, both in input order -- pdhip_simplify_mesh's output
 * contract: every output vertex is referenced.  out_vertices (device [Vn,3] f32) and, with colors [Vn,3] f32, out_colors: copies bit for bit;
 * out_faces (device [F,3] i64): the kept faces re-indexed; vertex_map (device [Vn] i32, may be NULL): the new index of every vertex, -1 for a dropped
 * one.  counts (device [4]): output vertices, output faces, 0, 0.  Two exclusive scans through the shared tiled scan; equal bytes on repeats.
 * ws: pdhip_compact_mesh_workspace_bytes(Vn, F) device bytes (0 for sizes the entry refuses).  PDHIP_E_ARG with the cause, and every output
 * untouched: a null pointer (named), colors without out_colors or the reverse, Vn < 1, F < 0, Vn > 2^26, F > 2^23, a face index outside [0, Vn)
 * (in a dropped face too).  The read of the check word SYNCHRONISES the stream once, after the last launch. */
size_t pdhip_compact_mesh_workspace_bytes(int Vn, int F);
int pdhip_compact_mesh(const float* vertices, int Vn, const int64_t* faces, int F, const float* colors_or_null, const uint8_t* face_keep,
                       float* out_vertices, int64_t* out_faces, float* out_colors_or_null, int32_t* vertex_map_or_null, int32_t* counts, void* ws,
                       void* stream);

/* ---- Taubin lambda | mu smoothing of a mesh with uniform ("umbrella") weights, and its boundary vertices (csrc/mesh_smooth.hip; no reference
 * counterpart: MeshLab's "Taubin Smooth").  Both entries work on the neighbour CSR of pdhip_neighbour_csr: rowptr (device [Vn+1] i32) and colidx
 * (device [rowptr[Vn]] i32), row v = the unique neighbours N(v) of vertex v, ascending, v itself not among them.  EVERY buffer is an argument the caller
 * allocates: there is no workspace and no size query.
 * pdhip_smooth_mesh: vertices (device [Vn,3] f32) -> out_vertices (device [Vn,3] f32); connectivity, and so faces and colours, are not touched.  The
 * state is f64, the input converted exactly.  One pass with factor s: a held vertex (held[v] != 0; held may be NULL) and a vertex with an empty row keep
 * their position; every other vertex gets x'[v] = x[v] + s * (m - x[v]), m = (sum of x[j], j in N(v)) / |N(v)|, per coordinate: the sum taken
 * sequentially in row order from 0.0, then one IEEE division, one subtraction, one multiplication, one addition, none of them fused.  Every vertex reads
 * the old state (Jacobi).  One step = a pass with lambda, then, if mu != 0, a pass with mu; after `steps` steps the state is rounded once to f32.  The
 * result is therefore bit-equal to that definition evaluated in numpy; it depends on the mesh only through the neighbour sets -- not on the order of the
 * faces, the rotation of a face's indices or the threads' order -- and two calls give equal bytes.  It is NOT invariant under relabelling the
 * vertices: the order of each sum follows the indices.  state_a, state_b (device [Vn,4] f64 each, 32-byte aligned, distinct): ping-pong scratch, the
 * fourth word of a row is padding; their contents before and after the call mean nothing.  counts (device [4] i32): vertices moved, held (with a
 * non-empty row), isolated (empty row), and the check word; they add up to Vn.  Launches: one check, then steps * (mu != 0 ? 2 : 1) passes, the first
 * reading `vertices`, the last writing out_vertices.
 * PDHIP_E_ARG with the cause, before any device call: a null pointer (named; only held may be NULL), Vn < 1, Vn > 2^26, steps < 1, steps > 10000,
 * lambda not in (0, 1], mu not finite or > 0, -lambda <= mu < 0 (not a Taubin pair: the pass band 1/lambda + 1/mu must be positive),
 * |(1 - 2 lambda)(1 - 2 mu)| > 1 (a step would amplify the highest frequency, k = 2, of the normalised umbrella operator), a state buffer that is not
 * 32-byte aligned, state_a == state_b.  mu == 0 is the plain Laplacian.  PDHIP_E_ARG from the check launch, out_vertices and the state buffers
 * untouched (counts is written): rowptr[0] != 0 or rowptr not monotone up to rowptr[Vn], a colidx outside [0, Vn), a vertex with a non-empty row that
 * is not finite.  The read of counts SYNCHRONISES the stream once, after the last launch (16 bytes).
 * pdhip_mesh_boundary_vertices: faces [F,3] i64 on the device and THEIR neighbour CSR.  An ordered pair (a, b), a != b, is a boundary pair when it
 * occurs exactly once among the 6 F ordered pairs of the faces (each edge of each face in both directions); a boundary vertex is one with a boundary
 * pair; an edge on three faces or more is not boundary.  pair_faces (device [rowptr[Vn]] i32): the occurrences of the pair (v, colidx[pos]);
 * boundary (device [Vn] u8): 1 for a boundary vertex; counts (device [4] i32): boundary vertices, boundary pairs / 2 (edges on one face), pairs on more
 * than two faces / 2, and the check word.  Integer atomics only: a function of the mesh alone, equal bytes on repeats.  PDHIP_E_ARG: a null pointer
 * (named), Vn < 1, F < 1, Vn > 2^26, F > 2^23; and from the device, boundary untouched (pair_faces is then undefined): rowptr not a CSR (rowptr[0] != 0,
 * not monotone, rowptr[Vn] > 6 F), a face index outside [0, Vn), a pair of a face that its row does not hold.  SYNCHRONISES once, after the last launch. */
int pdhip_mesh_boundary_vertices(const int64_t* faces, int F, int Vn, const int32_t* rowptr, const int32_t* colidx, int32_t* pair_faces,
                                 uint8_t* boundary, int32_t* counts, void* stream);
int pdhip_smooth_mesh(const float* vertices, int Vn, const int32_t* rowptr, const int32_t* colidx, const uint8_t* held_or_null, int steps,
                      double lambda, double mu, double* state_a, double* state_b, float* out_vertices, int32_t* counts, void* stream);

/* ---- welding of close vertices and cleaning of a face list (csrc/mesh_clean.hip; the reference gets both from trimesh's merge_vertices and
 * pymeshlab's "Merge Close Vertices", "Remove Duplicate Faces", "Remove Unreferenced Vertices").  The first step of the mesh chain for SUPPLIED meshes:
 * clean -> components -> smooth -> decimate -> unwrap -> texture.  EVERY buffer is an argument the caller allocates: there is no workspace and no size
 * query; each entry is told the length of every temporary and refuses a short one by name.
 * pdhip_weld_vertices: vertices (device [Vn,3] f32), tol (a finite double >= 0) -> rep (device [Vn] i32).  Vertices i and j are CLOSE when
 * d2(i, j) <= tol * tol, with d2 = (dx dx + dy dy) + dz dz on the f32 coordinates widened to f64, one rounding per operation, none fused (so
 * d2(i, j) == d2(j, i) bit for bit), and tol * tol one f64 product.  tol == 0 merges exactly equal coordinates; -0.0 equals +0.0.  A CLASS is a connected
 * component of the closeness graph (single linkage: a chain of close pairs is one class however long), rep[v] the smallest index of v's class.  rep
 * is a function of the vertex array alone -- not of the grid, the scan order or the threads' order -- and equals the all-pairs definition bit for bit
 * (mesh_clean.hip's header has the proof); two calls give equal bytes.  counts (device [4] i32): classes, vertices merged away (Vn - classes), cells per
 * axis of the grid, vertices whose scan needed more than the 27 cells around their own.  The grid: C^3 cubic cells over the vertices' box, C = min(
 * pdhip_weld_cells_axis(Vn) = clamp(floor(sqrt(Vn / 8)), 1, 256), floor(ext / (1.001 tol + 4e-12 max|coordinate|))), at least 1, ext = the box's
 * longest edge, cell edge ext / C * (1 + 1e-6): always larger than tol.  Temporaries (device; their contents before and after mean nothing):
 *   keys_a, keys_b [sort_len] u64 and vals_a, vals_b [sort_len] i32, sort_len >= Vn;  hist [hist_words] i32, hist_words >= 512 * ceil(Vn / 2048);
 *   cstart [cstart_len] i32, cstart_len >= pdhip_weld_cells_axis(Vn)^3 + 1;  sorted_xyzi [sorted_len, 4] f32, sorted_len >= Vn rows, 16-byte aligned;
 *   parent [parent_len] i32, parent_len >= Vn;  misc [misc_len] i32, misc_len >= 64.
 * Cost: every vertex visits the vertices of the cells around it, so n vertices in one cell cost n^2 steps or more (all vertices at one point:
 * Vn^2); nothing but Vn bounds it.  PDHIP_E_ARG with the cause, rep and counts untouched: a null pointer (named), Vn < 1, Vn > 2^26, tol negative,
 * NaN or infinite, a temporary that is too short (named, with both lengths), sorted_xyzi not 16-byte aligned, vertices with a non-finite coordinate
 * (their number is named).  SYNCHRONISES the stream twice: the read of the box (32 bytes), and the read of the check words after the last launch.
 * A union-find walk is bounded by 2 Vn + 64 steps; should one use them up, PDHIP_E_STATE.
 * pdhip_clean_faces: faces (device [F,3] i64) and rep (device [Vn] i32, pdhip_weld_vertices' output; the identity cleans without welding) ->
 * out_faces (device [F,3] i64): EVERY face with each index replaced by its representative, winding and corner order kept; keep (device [F] u8): 1 for
 * the faces that stay.  A face is DEGENERATE when two of its three new indices are equal; two non-degenerate faces are DUPLICATES when their sorted
 * index triples are equal (orientation ignored, as MeshLab does), and of each set of duplicates the smallest face index stays.  counts (device [4]
 * i32): degenerate, duplicate, kept, 0 (they add up to F).  pdhip_compact_mesh(vertices, out_faces, keep) then gives the cleaned mesh: surviving
 * faces in input order, the vertices they name -- representatives all -- in input order, the rest dropped.  Duplicates are found by a stable radix
 * sort of the key (lo, mid, hi), 21 bits each at most, with the face index as value.  Temporaries: keys_a, keys_b [sort_len] u64, vals_a, vals_b
 * [sort_len] i32, sort_len >= F; hist [hist_words] i32, hist_words >= 512 * ceil(F / 2048); misc [misc_len] i32, misc_len >= 64.  PDHIP_E_ARG with
 * the cause: a null pointer (named), Vn < 1, F < 1, Vn > 2^21 (both sizes named), F > 2^23, a short temporary (named); and from the device, out_faces
 * and keep untouched (counts is cleared): faces with an index outside [0, Vn), or whose rep lies outside [0, Vn) (their number is named).
 * SYNCHRONISES once, after the last launch (8 bytes).  Equal bytes on repeats. */
int pdhip_weld_cells_axis(int Vn);
int pdhip_weld_vertices(const float* vertices, int Vn, double tol, int32_t* rep, int32_t* counts, uint64_t* keys_a, uint64_t* keys_b, int32_t* vals_a,
                        int32_t* vals_b, size_t sort_len, int32_t* hist, size_t hist_words, int32_t* cstart, size_t cstart_len, float* sorted_xyzi,
                        size_t sorted_len, int32_t* parent, size_t parent_len, int32_t* misc, size_t misc_len, void* stream);
int pdhip_clean_faces(const int64_t* faces, int F, const int32_t* rep, int Vn, int64_t* out_faces, uint8_t* keep, int32_t* counts, uint64_t* keys_a,
                      uint64_t* keys_b, int32_t* vals_a, int32_t* vals_b, size_t sort_len, int32_t* hist, size_t hist_words, int32_t* misc,
                      size_t misc_len, void* stream);

/* ---- coherent orientation of a face list, patch by patch, closed patches outward (csrc/mesh_orient.hip; the reference gets it from its loaders:
 * trimesh.repair.fix_normals, pymeshlab's "Re-Orient all faces coherently").  The step behind the cleaning in the chain for SUPPLIED meshes:
 * clean -> orient -> components -> smooth -> decimate -> unwrap -> texture.  EVERY buffer is an argument the caller allocates: there is no workspace and
 * no size query; the entry is told the length of every temporary and refuses a short one by name.
 * pdhip_orient_faces: vertices (device [Vn,3] f32) and faces (device [F,3] i64, any indexed triangle list with indices in [0, Vn)).  Definitions:
 *   - A face with two equal indices is DEGENERATE: it has no edges, is never flipped and gets face_patch = -1.
 *   - Every other face f has three HALF-EDGES (a, b) = (f[k], f[(k + 1) % 3]), each with the undirected key {lo, hi} and the direction bit d = (a > b).
 *   - An edge is MANIFOLD when exactly two half-edges carry its key, BOUNDARY with one, NON-MANIFOLD with three or more.
 *   - Orientation crosses manifold edges only (as in MeshLab and trimesh).  The parity of a manifold edge is e = (d1 == d2): e = 1 means that its two
 *     faces traverse it in the same direction, so one of them must flip.
 *   - A PATCH is a connected component of the non-degenerate faces across manifold edges, its root its smallest face index; patches are numbered
 *     0 .. P - 1 by ascending root.
 *   - rel[f] is the XOR of the edge parities along any path from the root to f.  A patch is NON-ORIENTABLE when some manifold edge has
 *     rel[fa] ^ rel[fb] != e (the paths then disagree); none of its faces is flipped, its patch_flipped and patch_vol are 0.
 *   - A patch is CLOSED when none of its faces has a boundary or a non-manifold edge.
 *   - Per orientable patch flip[f] = rel[f] ^ c, with c from one of two rules.  The VOLUME rule applies to closed patches, and with open_patches == 1
 *     to every patch: the patch's box over the vertices its faces name, per axis lo and hi as f64; ext = the longest edge hi - lo of that box;
 *     s = 4095.0 / ext, one f64 division (s = 0 when ext == 0); q = clamp(floor(((double)x - lo) * s), 0, 4095) per coordinate (one subtraction, one
 *     product, none fused); the centred integer coordinate is 2 q - 4095; vol = the sum over the patch's faces AS GIVEN of (1 - 2 rel[f]) det(A, B, C)
 *     in int64 (|det| < 2^39 per face and F <= 2^23, so |vol| < 2^62: an integer sum, whatever its order).  vol < 0 gives c = 1, vol > 0 gives c = 0,
 *     vol == 0 falls through to the MAJORITY rule: c = 1 when more faces of the patch have rel = 1 than rel = 0 (the fewest flips); a tie gives c = 0,
 *     so the root keeps its winding.
 *   - A flipped face (a, b, c) becomes (a, c, b): the first corner stays, so per-face rows such as an OBJ's `ft` flip by the same swap.
 *   Every output is a function of the mesh alone: not of the order of the faces (except through "smallest index"), the rotation of a face's corners
 *   (flip, the patches and every count; out_faces keeps each face's own first corner) or the threads' order; two calls give equal bytes.  Nested
 *   cavities are NOT turned inward: each closed patch is turned outward on its own, as trimesh does for multibody meshes.  Nothing crosses a
 *   non-manifold edge, and no hole is filled.
 * Outputs (device): out_faces [F,3] i64 (every face, flipped or as given); flip [F] u8; face_patch [F] i32; per patch, entries [0, P) of arrays of F
 * elements each (the rest is not touched): patch_root, patch_faces, patch_flipped (faces of the patch that were flipped) i32, patch_flags i32 (1 closed,
 * 2 non-orientable, 4 decided by volume: the rule applied and vol != 0, 8 complemented: c = 1), patch_vol i64 (vol where the volume rule applied to an
 * orientable patch, else 0); counts [8] i32: patches, faces flipped, non-orientable patches, incoherent manifold edges as given (e = 1), boundary edges,
 * non-manifold edges, degenerate faces, 0.  open_patches: 0 = 'majority' (open patches by the majority rule), 1 = 'volume'.
 * Temporaries (device; their contents before and after mean nothing): keys_a, keys_b [sort_len] u64 and vals_a, vals_b [sort_len] i32,
 * sort_len >= 3 F (the half-edge table and its stable radix sort);  hist [hist_words] i32, hist_words >= 512 * ceil(3 F / 2048);  face_tmp
 * [face_tmp_len] i32, face_tmp_len >= 5 F (the parity union-find's words, root, root flag, patch id, the face bits);  box [box_len] i32,
 * box_len >= 6 F (the patch boxes in ordered bits);  tiles [tiles_len] i32, tiles_len >= 2 * (F / 2048 + 1) (the tiled scan's sums);  misc [misc_len]
 * i32, misc_len >= 64.  Integer atomics only, zero scratch.  1 <= Vn <= 2^26, 1 <= F <= 2^23.
 * PDHIP_E_ARG with the cause, every output untouched: a null pointer (named), sizes out of range, open_patches other than 0 and 1, a short temporary
 * (named, with both lengths); and from the device (the temporaries are written, no output is): a face index outside [0, Vn), a referenced vertex (of a
 * degenerate face too) that is not finite.  SYNCHRONISES the stream once, after the last launch (8 bytes).  Patches are found by the parity variant of
 * csrc/union_find.h: one word parent << 1 | parity per face, hooks by compare-and-swap, path halving by one 32-bit store; non-orientability is decided
 * by a later launch that re-checks every manifold edge.  A walk is bounded by 2 F + 64 steps; should one use them up, PDHIP_E_STATE. */
int pdhip_orient_faces(const float* vertices, int Vn, const int64_t* faces, int F, int open_patches, int64_t* out_faces, uint8_t* flip,
                       int32_t* face_patch, int32_t* patch_root, int32_t* patch_faces, int32_t* patch_flipped, int32_t* patch_flags, int64_t* patch_vol,
                       int32_t* counts, uint64_t* keys_a, uint64_t* keys_b, int32_t* vals_a, int32_t* vals_b, size_t sort_len, int32_t* hist,
                       size_t hist_words, int32_t* face_tmp, size_t face_tmp_len, int32_t* box, size_t box_len, int32_t* tiles, size_t tiles_len,
                       int32_t* misc, size_t misc_len, void* stream);

/* ---- test-only entries onto the shared device primitives (csrc/prims_debug.hip): the radix sort and the scans of csrc/radix_sort.h and the sort
 * half of csrc/cell_list.h, which every geometry unit that sorts or scans includes.  The kernels have internal linkage, so these entries run
 * prims_debug.hip's copy: the same source and the same flags as every consumer's.  Nothing the product calls (tests/test_gpu_prims.py).
 * pdhip_debug_prims_workspace_bytes(n, nc): the bytes of ONE layout that all three entries carve: the two key and the two value buffers of n elements
 * and the digit histograms of the sort, cstart [nc + 1] i32, and the tile sums / tile offsets of a tiled scan of n elements (8 bytes each).  0 for
 * n < 1, n > 2^26, nc < 1 or nc > 2^26.
 * pdhip_debug_radix_sort: keys (device [n] u64), vals (device [n] i32) -> keys_out, vals_out: radix_sort(bits) on copies of the inputs in the
 * workspace.  The order is STABLE and by the key bits [0, 8 * ceil(bits / 8)): whole 8-bit digits; bits above that are carried along unread, and
 * bits == 0 copies the inputs through.  0 <= bits <= 64.  ws: pdhip_debug_prims_workspace_bytes(n, 1) bytes.
 * pdhip_debug_sort_by_cell: keys (device [n] u64, key[i] = the cell of point i, < 2^bits_for(nc); a key >= nc is a point outside every cell) ->
 * keys_out [n] (the sorted keys), idx_out [n] i32 (the points' indices in that order: the stable argsort of keys), cstart_out [nc + 1] i32
 * (cstart[c] = the first sorted position whose key is >= c), as sort_by_cell gives them to its consumers.  ws: pdhip_debug_prims_workspace_bytes(n, nc).
 * pdhip_debug_scan: in -> out (device [n], elem_bytes 4 = int, 8 = uint64_t; the entry works on the caller's arrays themselves and writes out[0 .. n)
 * only).  mode 0: the one-workgroup k_scan; 1: the tiled scan_exclusive / scan_inclusive.  inclusive != 0: out[i] = in[0] + ... + in[i], else
 * ... + in[i - 1], sums modulo 2^32 / 2^64.  nc: the nc the workspace was sized with (cstart lies in front of the tile sums);
 * ws: pdhip_debug_prims_workspace_bytes(n, nc).
 * These three entries enqueue on `stream` and do not synchronise.  PDHIP_E_ARG with the cause, nothing launched: a null pointer (named), n < 1 or
 * n > 2^26, nc outside [1, 2^26], bits outside [0, 64], elem_bytes other than 4 and 8, mode other than 0 and 1.
 * pdhip_debug_union_pairs: the union-find of csrc/union_find.h, which mesh_components.hip, mesh_clean.hip and uv_atlas.hip share.  pairs (device
 * [n_pairs, 2] i32, indices in [0, n); may be NULL with n_pairs == 0) -> parent (device [n] i32, the caller's: the forest, left as the unions
 * made it), root (device [n] i32: the smallest index of the class of every vertex), status (device [1] i32: 0, or the OR of 1 = a union and
 * 2 = a walk used up its budget of steps; root then holds -1 where a walk ended).  Three steps: k_uf_identity; one thread per pair,
 * unite(find_root, find_root) with a budget of 2 n + 64 steps; one thread per vertex, walk_root with n steps.  1 <= n <= 2^26,
 * 0 <= n_pairs <= 2^26; no workspace.  With n_pairs > 0 it SYNCHRONISES once before the unions (4 bytes: the pairs with an index outside
 * [0, n) are counted on the device, and any is PDHIP_E_ARG before parent is touched).
 * pdhip_debug_parity_union: the parity variant of that union-find, which mesh_orient.hip uses.  pairs (device [n_pairs, 2] i32) and parity (device
 * [n_pairs] u8, 0 or 1: pair p says rel[a] ^ rel[b] == parity[p]; both may be NULL with n_pairs == 0) -> word (device [n] i32, the caller's: the
 * forest, parent << 1 | parity, left as the unions made it), root (device [n] i32: the smallest index of every node's class), rel (device [n] u8: the
 * parity of the node relative to its root along the forest; a function of the pairs alone in a class without conflict), conflict (device [n] u8: 1 for
 * every node of a class in which some pair contradicts the forest's relations, i.e. which has no 2-colouring; decided by a launch that re-checks every
 * pair after the unions, so it does not depend on the threads' order), status as above.  Five steps: k_ufp_identity; one thread per pair,
 * unite_parity(find_root_parity, find_root_parity) with a budget of 2 n + 64 steps; one thread per node, walk_root_parity with n steps; the re-check;
 * the spread of the flag from the roots.  Limits, the synchronisation and the refusals as pdhip_debug_union_pairs; a parity above 1 is refused too. */
size_t pdhip_debug_prims_workspace_bytes(int n, int nc);
int pdhip_debug_radix_sort(const uint64_t* keys, const int32_t* vals, int n, int bits, uint64_t* keys_out, int32_t* vals_out, void* ws, void* stream);
int pdhip_debug_sort_by_cell(const uint64_t* keys, int n, int nc, uint64_t* keys_out, int32_t* idx_out, int32_t* cstart_out, void* ws, void* stream);
int pdhip_debug_scan(const void* in, void* out, int n, int elem_bytes, int mode, int inclusive, int nc, void* ws, void* stream);
int pdhip_debug_union_pairs(const int32_t* pairs, int n_pairs, int n, int32_t* parent, int32_t* root, int32_t* status, void* stream);
int pdhip_debug_parity_union(const int32_t* pairs, const uint8_t* parity, int n_pairs, int n, int32_t* word, int32_t* root, uint8_t* rel,
                             uint8_t* conflict, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
