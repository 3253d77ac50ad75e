/* harp_hip.h — C ABI of libharp_hip.so: the MI355X (gfx950) kernels of HARP's render-and-compare hot path.
 *
 * The reference (korrawe/harp) has no FFI layer of its own: its hot path reaches native code through PyTorch3D's
 * torch-extension ops and torch operators.  Each entry point below names the reference call site(s) it replaces
 * (paths relative to the reference repo) — this is what a maintainer would bind.
 *
 * Conventions: plain device pointers + sizes; float32 / int32, contiguous row-major; no hidden allocation (outputs and
 * workspaces are caller-provided); every call only enqueues work on `stream` (hipStream_t passed as void*-compatible
 * handle) and returns 0 on success (1 = bad argument, 2+hipError = launch failure, 1000 = RCCL not found, 1001+ncclResult = RCCL
 * error); nothing throws across the ABI.
 * "(+=)" marks accumulate-into outputs (caller zero-initialises).
 */
#ifndef HARP_HIP_H
#define HARP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

/* ---- rasteriser -------------------------------------------------------------------------------------------------
 * replaces pytorch3d _C.rasterize_meshes (+ SoftSilhouetteShader / sigmoid_alpha_blend when soft != 0):
 *   MeshRasterizer built at renderer/renderer_helper.py:52-55 (K=50, blur), :76-79 and :444-447 (K=1), invoked at
 *   :344 (light view) and :353 (camera view); SoftSilhouetteShader at :56.
 * ndc (B,V,3) = (x_ndc, y_ndc, z_view) from harp_project_fwd; faces (F,3) shared by all frames.
 * outputs (B,S,S): face_id (frame-local face index of the nearest face, -1 = empty), zbuf (NULL ok; -1 = empty),
 * alpha (soft only).  ws: harp_rasterize_ws_bytes(B,F,S) bytes, 256-B aligned, kept until the backward calls ran. */
size_t harp_rasterize_ws_bytes(int B, int F, int S);
int harp_rasterize_fwd(const float* ndc, const int32_t* faces, int B, int V, int F, int S, int soft, float blur_radius,
                       float sigma, void* ws, int32_t* face_id, float* zbuf, float* alpha, hipStream_t stream);
/* The set-up part of the rasteriser calls below (face records with the blur-dilated bbox, per-super-tile face lists, launch order:
 * PyTorch3D's coarse rasterisation, renderer/renderer_helper.py:52-58, :344, :353) for TWO views of the same meshes in three launches
 * instead of six.  A rasteriser call on a workspace prepared here passes bit 2 (value 4) in its `soft` / `sparse` argument and then only
 * launches its tile pass.  blur_radius_x = the blur_radius of that view's pass (0 for a hard K = 1 pass). */
int harp_raster_setup_pair(const float* ndc_a, float blur_radius_a, void* ws_a, const float* ndc_b, float blur_radius_b, void* ws_b,
                           const int32_t* faces, int B, int V, int F, int S, hipStream_t stream);
/* K = 1 depth pass (the light view, renderer_helper.py:344) into a depth map zbuf that the caller KEEPS between calls.  st_state:
 * B * ceil(S/64)^2 ints, zero before the first call and owned by the library afterwards — which 64x64 super-tiles of zbuf hold -1
 * everywhere.  With sparse != 0 (face ids of super-tiles without a face are not written, as with soft bit 1 of harp_rasterize_fwd) a
 * super-tile that is empty again is not filled again: in a fitting step that is 3/4 of the map.  Nobody else may write zbuf between calls. */
int harp_rasterize_fwd_keep(const float* ndc, const int32_t* faces, int B, int V, int F, int S, int sparse, void* ws, int32_t* face_id,
                            float* zbuf, int32_t* st_state, hipStream_t stream);
/* the same with torch.nn.L1Loss(y_sil_true, y_sil_pred) (optimize_sequence.py:519) fused into the raster epilogue: l1_target (T,S,S)
 * indexed by l1_fid (B,), *l1_loss (+=) the mean, l1_grad (B,S,S) = l1_w[0] * d loss / d alpha.  l1_target == NULL: plain rasterisation. */
/* soft bit 0: soft silhouette on.  soft bit 1 (value 2): SPARSE outputs — face_id / alpha / l1_grad are left unwritten in 64x64
 * super-tiles that hold no face (their contribution to the loss is still accumulated; zbuf is always written everywhere).  For callers whose consumers skip those super-tiles too
 * (harp_shade_*, harp_silhouette_bwd do): 3/4 of a hand image is such background. */
/* l1_bg_sums (optional, used with sparse outputs): (T, nsx*nsx) per target frame and 64x64 super-tile, the term's sum over the
 * super-tile when nothing is rendered there (sum of y_sil) — targets are static during a fit, so the background part of the loss is
 * a table look-up instead of a pass over 3/4 of the target image every step. */
/* face_id == NULL (with the soft silhouette on and zbuf == NULL): silhouette only — the nearest face per pixel is neither formed nor
 * written (the geometry-only stage of a fit reads alpha alone). */
int harp_rasterize_l1_fwd(const float* ndc, const int32_t* faces, int B, int V, int F, int S, int soft, float blur_radius,
                          float sigma, void* ws, int32_t* face_id, float* zbuf, float* alpha, const float* l1_target,
                          const int32_t* l1_fid, const float* l1_w, float* l1_loss, float* l1_grad, const float* l1_bg_sums,
                          hipStream_t stream);
/* harp_rasterize_l1_fwd (soft & 1, y_sil != NULL) with the silhouette backward fused into the SAME launch (renderer_helper.py:44-58 forward,
 * rasterize_meshes_backward's dists path + sigmoid_alpha_blend's backward): g_ndc (B,V,3) += d (w * L1(alpha, y_sil)) / d ndc, x and y
 * components — what harp_silhouette_bwd(alpha, g_alpha) of the same workspace would add.  A tile's rim pixels walk the tile's faces again
 * while these are still staged in LDS; no second launch re-reads alpha / g_alpha and re-stages the lists.  alpha and g_alpha are still written. */
int harp_rasterize_l1_fwd_bwd(const float* ndc, const int32_t* faces, int B, int V, int F, int S, int soft, float blur_radius, float sigma,
                              void* ws, int32_t* face_id, float* alpha, const float* y_sil, const int32_t* fid, const float* w, float* loss,
                              float* g_alpha, const float* bg_sums, float* g_ndc, hipStream_t stream);
/* replaces _C.rasterize_meshes_backward (grad_dists path) + sigmoid_alpha_blend backward; g_ndc (B,V,3) (+=) */
int harp_silhouette_bwd(const int32_t* faces, int B, int V, int F, int S, float blur_radius, float sigma, const void* ws,
                        const float* alpha, const float* g_alpha, float* g_ndc, hipStream_t stream);
/* Silhouette records: the soft pass of the camera view (renderer_helper.py:44-58) already pairs every pixel it blends with every face
 * whose soft factor it forms — the pairs that rasterize_meshes_backward's dists path (with sigmoid_alpha_blend's backward) differentiates.
 * harp_sil_records_bind(ws, sil_rec, rec_cap, B, F, S) binds a record buffer of harp_sil_records_bytes(B, S, rec_cap) bytes to a
 * workspace: from then on every soft pass on ws (harp_rasterize_fwd / harp_rasterize_l1_fwd with soft & 1, up to B frames of S^2) also
 * stores its pairs there — per (frame, 16x16 tile) a count and up to rec_cap records (face id << 8 | pixel of the tile; a tile with more
 * stores its count only) — and harp_silhouette_bwd on ws walks those pairs instead of finding them again (a tile over the capacity walks
 * as without records).  Every output of both calls is what it is without records (the gradient up to the order of float sums).  Keep the
 * binding between a forward and its backward; sil_rec needs no initial contents.  sil_rec == NULL unbinds.  Host-side state, read when a
 * call is enqueued (a captured graph replays what was bound at capture). */
size_t harp_sil_records_bytes(int B, int S, int rec_cap);
int harp_sil_records_bind(const void* ws, void* sil_rec, int rec_cap, int B, int F, int S);
/* replaces _C.rasterize_meshes_backward (grad_zbuf path) for a K=1 pass: g_z (B,S,S) -> g_ndc (B,V,3) (+=) */
int harp_depth_bwd(const int32_t* face_id, const void* ws, const int32_t* faces, const float* g_z, int B, int V, int F, int S,
                   float* g_ndc, hipStream_t stream);
/* the same for a caller that keeps ONE gradient image g_z across steps (the fitting loop: harp_shade_bwd scatters the shadow test's tap
 * gradients of renderer_helper.py:385-408 into it): every non-zero entry read is also cleared.  The shader only ever writes at light-view
 * pixels that hold a face (an empty texel's depth -1 gives a shadow-test sigmoid of exactly 0), all of which this pass visits, so an
 * image that was all-zero before the step's harp_shade_bwd is all-zero again after this call and needs no per-step clear. */
int harp_depth_bwd_consume(const int32_t* face_id, const void* ws, const int32_t* faces, float* g_z, int B, int V, int F, int S,
                           float* g_ndc, hipStream_t stream);
/* harp_depth_bwd_consume + harp_normalize3_bwd(nmap, g_nmap_n, n_texels, g_nmap) as ONE launch: the two small passes between the shader
 * backward and the per-frame backward tail of a fitting step (neither reads what the other writes) */
int harp_depth_nmap_bwd(const int32_t* face_id, const void* ws, const int32_t* faces, float* g_z, int B, int V, int F, int S, float* g_ndc,
                        const float* nmap, const float* g_nmap_n, int n_texels, float* g_nmap, unsigned char* g_z_tiles, hipStream_t stream);
/* harp_depth_bwd_consume restricted to the tiles flagged in g_z_tiles (harp_shade_args.g_zl_tiles of the backward that filled g_z; NULL:
 * every tile); the flags of the tiles visited are cleared */
/* g_vert9 (n_verts, 9) of harp_shade_args -> g_verts / g_vnormals / g_ndc (n_verts,3 each) +=, g_vert9 all-zero again */
int harp_vert9_unpack(float* g_vert9, int n_verts, float* g_verts, float* g_vnormals, float* g_ndc, hipStream_t stream);
/* harp_depth_bwd_tiles (g_z consumed; g_z_tiles optional) with up to two riders in the SAME launch (extra workgroups behind the tile workgroups:
 * both only need the shader backward's output): nmap != NULL: harp_normalize3_bwd(nmap, g_nmap_n, n_texels, g_nmap); g_vert9 != NULL:
 * harp_vert9_unpack(g_vert9, B * V, g_verts, g_vnormals, g_ndc_cam). */
int harp_depth_bwd_riders(const int32_t* face_id, const void* ws, const int32_t* faces, float* g_z, int B, int V, int F, int S, float* g_ndc,
                          unsigned char* g_z_tiles, const float* nmap, const float* g_nmap_n, int n_texels, float* g_nmap, float* g_vert9,
                          float* g_verts, float* g_vnormals, float* g_ndc_cam, hipStream_t stream);
int harp_depth_bwd_tiles(const int32_t* face_id, const void* ws, const int32_t* faces, float* g_z, int B, int V, int F, int S,
                         float* g_ndc, unsigned char* g_z_tiles, hipStream_t stream);

/* ---- fragment-level rasterisation (the PyTorch3D op pair itself; NOT on the fitting loop's path) -----------------------------
 * replaces _C.rasterize_meshes(face_verts, mesh_to_face_first_idx, num_faces_per_mesh, clipped_faces_neighbor_idx, image_size,
 *   blur_radius, faces_per_pixel, bin_size, max_faces_per_bin, perspective_correct=True, clip_barycentric_coords=(blur_radius>0),
 *   cull_backfaces=False) -> (pix_to_face, zbuf, bary, dists) and _C.rasterize_meshes_backward(face_verts, pix_to_face, grad_zbuf,
 *   grad_bary, grad_dists, perspective_correct, clip_barycentric_coords) -> grad_face_verts, as reached through MeshRasterizer at
 *   renderer/renderer_helper.py:52-55 (K=50, blur), :76-79 (K=1), :88-101 (K=10 normal renderer), :444-447.
 * For callers that keep PyTorch3D-style shader classes.  K = faces_per_pixel is a CAP (1 <= K <= 64): the K nearest candidates are
 * kept in ascending depth, ties keep the lower face index.  Outputs (B,S,S,K): pix_to_face int32 frame-local (-1 = empty slot; the
 * PyTorch3D "packed" index is b*F + f), zbuf, bary (B,S,S,K,3), dists (signed squared NDC distance to the nearest edge); empty slots
 * hold -1 everywhere.  ws: harp_rasterize_ws_bytes(B,F,S).  Backward: any of g_zbuf / g_bary / g_dists may be NULL; g_ndc (+=); an
 * empty slot (pix_to_face < 0) contributes nothing, whatever its cotangents hold.  Both return HARP_ERR_ARG without a launch for a
 * NULL required pointer, B / V / S (forward: F) < 1, K outside 1..64, and a blur_radius that is negative, NaN or infinite. */
int harp_rasterize_fragments_fwd(const float* ndc, const int32_t* faces, int B, int V, int F, int S, float blur_radius, int K, void* ws,
                                 int32_t* pix_to_face, float* zbuf, float* bary, float* dists, hipStream_t stream);
int harp_rasterize_fragments_bwd(const float* ndc, const int32_t* faces, const int32_t* pix_to_face, const float* g_zbuf,
                                 const float* g_bary, const float* g_dists, int B, int V, int F, int S, float blur_radius, int K,
                                 float* g_ndc, hipStream_t stream);

/* ---- shader --------------------------------------------------------------------------------------------------------
 * replaces SoftPhongShaderShadow.forward + phong_shading_with_shadow + the shadow-map test of
 * MeshRendererShadow.forward (renderer/renderer_helper.py:360-408, 472-523, 565-592), PBRMaterials.apply_normal_map
 * (renderer/pbr_materials.py:58-124), TexturesUV.sample_textures, interpolate_face_attributes, _apply_lighting and
 * softmax_rgb_blend; with zl == NULL it is SoftPhongShaderPBR / phong_shading_PBR (renderer_helper.py:106-190). */
typedef struct harp_shade_args {
  /* geometry of the camera-view K=1 pass */
  const int32_t* face_id;   /* (B,S,S) from harp_rasterize_fwd */
  const void* recs;         /* the workspace of that call */
  const int32_t* faces;     /* (F,3) */
  const int32_t* faces_uvs; /* (F,3) */
  const float* verts_uvs;   /* (VT,2) */
  const float* verts;       /* (B,V,3) world */
  const float* vnormals;    /* (B,V,3) unit vertex normals */
  /* appearance */
  const float* tex;         /* (Ht,Wt,3) albedo */
  const float* nmap;        /* (Ht,Wt,3) per-texel normalised normal map, or NULL */
  const float* light_pos;   /* (B,3) */
  const float* colors;      /* 9 floats on device: ambient rgb, diffuse rgb, specular rgb (light x material) */
  /* self shadow (NULL zl => no shadow term) */
  const float* zl;          /* (B,S,S) light-view depth map (-1 empty) */
  const float* light_R;     /* (B,9) row-major, X_view = X R + T */
  const float* light_T;     /* (B,3) */
  int B, V, F, S, Ht, Wt;
  float focal, ppx, ppy;
  float bg[3];
  float* rgb;               /* out (B,S,S,3); may be NULL when l1_target is set: the loss and its gradient are produced without
                             * materialising the image (4 MB per 512x512 frame that nothing in an optimisation step reads back) */
  /* backward only */
  const float* g_rgb;       /* (B,S,S,3) */
  float* g_tex;             /* (Ht,Wt,3) (+=) or NULL */
  float* g_nmap;            /* (Ht,Wt,3) (+=) or NULL */
  float* g_verts;           /* (B,V,3) (+=) */
  float* g_vnormals;        /* (B,V,3) (+=) */
  float* g_ndc;             /* (B,V,3) (+=) camera-view NDC vertices.  harp_shade_bwd: all three NULL = no geometry gradients (the
                             * appearance-only stage, optimize_sequence.py:264-310: opt_app holds texture, normal map, light, ambient ratio) */
  float* g_zl;              /* (B,S,S) (+=) or NULL; see g_zl_tiles at the end of the struct */
  float* g_light_pos;       /* (B,3) (+=) or NULL */
  float* g_colors;          /* 9 (+=) or NULL */
  float* g_light_R;         /* (B,9) (+=) or NULL */
  float* g_light_T;         /* (B,3) (+=) or NULL */
  int debug_skip;           /* 0 in production (wave-autonomous backward kernel, csrc/shade_bwd.hip).  Non-zero selects the first,
                             * barrier-synchronised backward kernel: 64 = that kernel unmodified (A/B timing, same results); bits 0-5 are
                             * its ablation switches (tools/dev/gpu_shade_r3.py): 1/2 no texel adds, 4 no shadow-tap gradient, 8 no vertex
                             * adds, 16 no texel flush, 32 no vertex flush — results are then WRONG by design.  Bits 8-13 are the same kind of
                             * switches for the production kernel: 256 no texel phase, 512 no shadow window, 1024 no vertex phase, 2048 no table
                             * flushes, 8192 no shading at all (fixed cost of the launch) */
  /* forward only, optional: fused photometric L1 (optimize_sequence.py:543): *l1_loss (+=) mean |y_pred*m - y_true[fid]*m|,
   * l1_grad (B,S,S,3) = l1_w[0] * d loss / d y_pred, WRITTEN ONLY AT COVERED PIXELS (face_id >= 0: the only ones harp_shade_bwd reads).
   * l1_target == NULL disables it. */
  const float* l1_target;   /* (T,S,S,3) */
  const float* l1_mask;     /* (T,S,S) or NULL */
  const int32_t* l1_fid;    /* (B,) */
  const float* l1_w;
  float* l1_loss;
  float* l1_grad;
  float l1_inv;             /* filled in by harp_shade_fwd */
  /* optional (fwd and bwd): the SAME tex / nmap interleaved by harp_pack_texels; halves the cache lines of the bilinear footprint */
  const void* texnm;
  /* optional, used when rgb == NULL: (T, nsx*nsx) per target frame and 64x64 super-tile, sum over its pixels and channels of
   * |bg_c - y_c| * mask — the photometric term of a super-tile that holds no face (static targets: a table instead of reading mask
   * and target of 3/4 of the image every step) */
  const float* l1_bg_sums;
  /* optional (backward): (B, ceil(S/16), ceil(S/16)) bytes; the byte of every 16x16 light-view tile in which the backward adds to g_zl
   * is set to 1.  harp_depth_bwd_tiles / harp_depth_nmap_bwd read them to leave out the tiles without a gradient (about half of the
   * tiles they would otherwise read) and clear the ones they consume. */
  unsigned char* g_zl_tiles;
  /* optional (harp_shade_bwd, production kernel): texel-gradient RECORDS.  With trec != NULL the pass does not scatter the bilinear
   * footprints of g_tex / g_nmap (the backward of TexturesUV.sample_textures, renderer/pbr_materials.py:82-124) itself: every shaded
   * pixel appends ONE 36-byte record (texel x0 | y0 << 16, the two bilinear fractions, g_albedo[3], g_nmap[3]) to the list of the
   * 32x32-texel UV tile its top-left texel lies in, and harp_texel_reduce (below) adds the lists up tile by tile in LDS into the double
   * maps trec_acc_tex / trec_acc_nmap, which harp_texel_finish turns into g_tex / g_nmap.  harp_shade_bwd itself leaves g_tex / g_nmap
   * untouched (they still say WHICH maps take a gradient: NULL = frozen); a record that does not fit its list is added to the double maps
   * with memory atomics straight away.
   *   trec      (harp_texel_bins(Ht, Wt), 9, trec_cap) floats, plane k of bin b at ((b * 9 + k) * trec_cap); 16-byte aligned, trec_cap a
   *             multiple of 4
   *   trec_cnt  harp_texel_bins(Ht, Wt) * 16 + 16 int32: the record count of bin b at [16 b] (one counter per 64-byte line), ALL ZERO on
   *             entry; harp_texel_reduce hands them back zeroed */
  float* trec;
  int32_t* trec_cnt;
  int trec_cap;
  double* trec_acc_tex;    /* (Ht,Wt,3) doubles, the accumulators harp_texel_reduce adds into (required with trec unless the map is frozen) */
  double* trec_acc_nmap;
  /* optional (harp_shade_bwd, production kernel): (B,V,9) (+=).  The three vertex gradients go HERE instead of into g_verts / g_vnormals /
   * g_ndc, interleaved per vertex [g_verts(3) | g_vnormals(3) | g_ndc(3)]: a wave's table flush is then one 36-byte run per vertex instead of
   * three 12-byte runs in three arrays — a third of the memory-atomic lines.  g_verts / g_vnormals / g_ndc must still be non-NULL (they say
   * that geometry gradients are wanted) and stay untouched; harp_vert9_unpack or harp_depth_bwd_riders adds the buffer into them and clears it. */
  float* g_vert9;
} harp_shade_args;
/* number of 32x32-texel UV tiles (record bins) of an (Ht, Wt) map */
int harp_texel_bins(int Ht, int Wt);
/* second half of the texel gradient (see harp_shade_args.trec): acc_tex / acc_nmap (Ht,Wt,3) DOUBLE += the bilinear footprints of the
 * records the harp_shade_bwd call(s) since the last reduce appended.  One workgroup per chunk of 2048 records of a bin: a (33 x 33 texel) x
 * 6 channel 64-bit fixed-point accumulator in LDS (the extra row / column takes the footprints of the tile's last row / column; sums
 * exact and independent of the order of the records), added to the double maps with row-contiguous memory atomics — the gradient a texel
 * ends up with is float(exact sum) however the frames were batched.  Either map pointer may be NULL (frozen map).  The counters are
 * all-zero again when the call has run.  expected_records: a hint for the launch shape only (<= 2 M or <= 0: one workgroup per CU, which leaves
 * LDS for the kernels that run beside it; more: two) — e.g. a sixth of B * S * S. */
int harp_texel_reduce(const float* trec, int32_t* trec_cnt, int trec_cap, int Ht, int Wt, double* acc_tex, double* acc_nmap, int expected_records,
                      hipStream_t stream);
/* third and last part: g_tex (n_texels,3) += float(acc_tex), g_nmap += float(acc_nmap) — with nmap_raw != NULL through the chain rule of
 * F.normalize(nmap_raw, dim=-1) (utils/visualize.py:99; harp_normalize3_bwd's arithmetic: acc_nmap is then the gradient of the NORMALISED
 * map, g_nmap that of the raw one) — and both accumulators are all-zero again.  A NULL accumulator skips that map. */
int harp_texel_finish(double* acc_tex, float* g_tex, double* acc_nmap, float* g_nmap, const float* nmap_raw, int n_texels, hipStream_t stream);
/* interleaves albedo (Ht*Wt,3) and the normalised normal map (Ht*Wt,3) into out (Ht*Wt,8): [r g b nx | ny nz 0 0], 16-B aligned */
int harp_pack_texels(const float* tex, const float* nmap, int n_texels, float* out, hipStream_t stream);
/* harp_normalize3_fwd(nmap_raw) -> nmap_n and harp_pack_texels(tex, nmap_n) -> packed (may be NULL) in ONE launch */
int harp_normalize3_pack(const float* tex, const float* nmap_raw, int n_texels, float* nmap_n, float* packed, hipStream_t stream);
int harp_shade_fwd(const harp_shade_args* a, hipStream_t stream);
/* backward of the shading pass.  g_rgb != NULL: plain backward of an upstream gradient image.  g_rgb == NULL (FUSED-LOSS mode, needs
 * l1_target / l1_fid / l1_w / l1_loss / l1_bg_sums): no harp_shade_fwd call is needed at all — the pass recomputes the colour anyway,
 * forms torch.nn.L1Loss(y_true * m, y_pred * m) (optimize_sequence.py:543) and its gradient itself and accumulates the loss value;
 * with a->rgb != NULL it also writes that colour, i.e. the whole rendered image y_pred (background included), as harp_shade_fwd would. */
int harp_shade_bwd(const harp_shade_args* a, hipStream_t stream);
/* harp_shade_bwd(a) and harp_silhouette_bwd(a->faces, ..., ws = a->recs, alpha, g_alpha, g_ndc = a->g_ndc) of the SAME camera-view
 * rasterisation as ONE launch whose workgroups alternate between the two kinds of tile: as separate kernels on two streams they cannot
 * share a CU (registers / LDS), in one grid the rasteriser's waves issue while the shader's wait on memory.  Same results.  (a->trec is
 * ignored: this launch hosts the table form of the shader tile, the texel gradients go straight into g_tex / g_nmap.) */
int harp_shade_sil_bwd(const harp_shade_args* a, float blur_radius, float sigma, const float* alpha, const float* g_alpha,
                       hipStream_t stream);

/* ---- mesh preparation --------------------------------------------------------------------------------------------
 * replaces the PyTorch3D object churn of utils/visualize.py:prepare_mesh (:45-64): Meshes(...), SubdivideMeshes
 * (optimize_sequence.py:67-89), verts_normals_padded, displacement; and Meshes.verts_normals_packed in the shaders
 * (renderer_helper.py:495).  CSR tables come from harp_amd/topology.py.  Every call below returns HARP_ERR_ARG without launching
 * for a NULL input or output table, B <= 0, V <= 0 or V0 <= 0 (E0 < 0, V < V0 for the subdivision).  Accumulating outputs (+=):
 * g_v of harp_vertex_normals_bwd and harp_project_bwd, g_R / g_T of harp_project_bwd (each may be NULL), g_disp of
 * harp_displace_bwd (summed over the batch); g_n of harp_displace_bwd is overwritten. */
int harp_subdivide_fwd(const float* v0, const int32_t* edges0, int B, int V0, int E0, float scale, float* vs, hipStream_t stream);
int harp_subdivide_bwd(const float* g_vs, const int32_t* sub_off, const int32_t* sub_idx, int B, int V0, int V, float scale,
                       float* g_v0, hipStream_t stream);
int harp_vertex_normals_fwd(const float* v, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_idx, int B, int V,
                            float* n, float* inv_len, const float* disp, float* vd, hipStream_t stream);
int harp_vertex_normals_bwd(const float* v, const int32_t* faces, const int32_t* vf_off, const int32_t* vf_idx, int B, int V,
                            const float* n, const float* inv_len, const float* g_n, float* tmp, float* g_v, hipStream_t stream);
int harp_displace_bwd(const float* g_vd, const float* n, const float* disp, int B, int V, float* g_n, float* g_disp,
                      hipStream_t stream);
/* replaces MeshRasterizer.transform with PerspectiveCameras(in_ndc=False) (call sites utils/visualize.py:272-279, 304-313) */
int harp_project_fwd(const float* v, const float* R, const float* T, int B, int V, float focal, float ppx, float ppy, int S,
                     float* ndc, hipStream_t stream);
int harp_project_bwd(const float* v, const float* R, const float* T, const float* g_ndc, int B, int V, float focal, int S,
                     float* g_v, float* g_R, float* g_T, hipStream_t stream);
/* hand_verts.mean(1) (optimize_sequence.py:476) */
int harp_centroid(const float* v, int B, int V, float* c, hipStream_t stream);

/* ---- MANO linear-blend skinning ----------------------------------------------------------------------------------
 * replaces ManoLayer.forward (manopth/manolayer.py:108-296, rodrigues_layer.py:15-54, tensutils.py:6-42) as built by
 * utils/hand_model_utils.py:74 (use_pca=False, flat_hand_mean=False, axis-angle root, right hand); call site
 * utils/visualize.py:42-44.  Model arrays are device pointers prepared once by harp_amd/manopth/manolayer.py. */
typedef struct harp_mano_model {
  const float* v_template;   /* (778,3) */
  const float* shapedirs_T;  /* (10, 778*3)  th_shapedirs transposed */
  const float* posedirs_T;   /* (135, 778*3) th_posedirs transposed */
  const float* posedirs;     /* (778*3, 135) */
  const float* J_template;   /* (16,3)  = J_regressor @ v_template */
  const float* J_dirs;       /* (16*3,10) = J_regressor @ shapedirs */
  const float* weights;      /* (778,16) */
  const float* hands_mean;   /* (45,) */
} harp_mano_model;
size_t harp_lbs_mano_ws_floats(int B);
/* pose (B,48) = [root axis-angle, 45 hand pose], betas (B,10), trans (B,3) -> verts (B,778,3) mm, joints (B,21,3) mm */
int harp_lbs_mano_fwd(const harp_mano_model* m, const float* pose, const float* betas, const float* trans, int B, float* ws,
                      float* verts, float* joints, hipStream_t stream);
/* ws must be the workspace of the forward call; g_verts is modified in place (tip-joint gradients folded in: g_verts[tip] +=
 * g_joints[tip joint]); g_pose, g_betas and g_trans are overwritten.  The call may be repeated on one forward workspace (with the
 * original g_verts each time).  B <= 0 returns HARP_ERR_ARG without launching (harp_lbs_mano_fwd likewise). */
int harp_lbs_mano_bwd(const harp_mano_model* m, const float* pose, const float* betas, const float* trans, int B, float* ws,
                      float* g_verts, const float* g_joints, float* g_pose, float* g_betas, float* g_trans, hipStream_t stream);

/* ---- kinematic-tree LBS (SMPL-X right arm) ------------------------------------------------------------------------
 * replaces SMPLXARM.forward(..., return_type='mano_w_arm') (hand_models_harp/body_models.py:2163-2390: smplx.lbs :2335, recentre on
 * the right wrist :2342-2343, transl :2378-2380, arm slice :2383-2390); call site utils/visualize.py:37-40.  The model is sliced
 * to the arm vertices on the host (harp_amd/hand_models_harp/body_models.py), the joint regressor folded into J_template/J_dirs. */
typedef struct harp_tree_model {
  int NV, NJ, NB;              /* vertices kept, joints (<= 64), shape coefficients (<= 32) */
  const float* v_template;     /* (NV,3) */
  const float* shapedirs_T;    /* (NB, NV*3) */
  const float* posedirs_T;     /* ((NJ-1)*9, NV*3)  (smplx layout) */
  const float* posedirs;       /* (NV*3, (NJ-1)*9) */
  const float* J_template;     /* (NJ,3) */
  const float* J_dirs;         /* (NJ*3, NB) */
  const float* weights;        /* (NV,NJ) */
  const float* pose_mean;      /* (NJ*3) */
  const int32_t* parents;      /* (NJ) parents[0] = -1, parents[j] < j */
  const int32_t* pose_src;     /* (NJ) row of in_pose driving joint j, or -1 (axis-angle = pose_mean only) */
  int n_pose_in;               /* rows of in_pose: (B, n_pose_in, 3) = [global_orient, right_wrist_pose, right_hand_pose(15)] */
  int center_joint;            /* recentre on this chain joint (21 = right wrist) or -1 */
  int n_joints_out;            /* 22 */
  const int32_t* joint_src;    /* (n_joints_out): >= 0 chain joint id, < 0: vertex joint -(vertex id)-1 */
} harp_tree_model;
size_t harp_lbs_tree_ws_floats(const harp_tree_model* m, int B);
/* verts (B,NV,3) mm, joints (B,n_joints_out,3) mm */
int harp_lbs_tree_fwd(const harp_tree_model* m, const float* in_pose, const float* betas, const float* transl, int B, float* ws,
                      float* verts, float* joints, hipStream_t stream);
/* ws: the workspace harp_lbs_tree_fwd filled for the same inputs AND THE SAME B (the layout of ws is a function of B).  The forward call
 * clears the accumulators this call adds to, and this call leaves them cleared again: it may be repeated on one forward pass, and a
 * workspace may be reused for another batch size by running harp_lbs_tree_fwd at that size first.  Calling it on a workspace whose last
 * forward ran at another B, or that the caller filled itself, accumulates into whatever those bytes hold.  g_verts is modified in place
 * (vertex-joint gradients folded in: g_verts[vertex] += g_joints[its joint]); g_in_pose (the rows pose_src names), g_betas and g_transl are overwritten.
 * B <= 0, NJ > 64 or NB > 32 return HARP_ERR_ARG without launching (harp_lbs_tree_fwd likewise). */
int harp_lbs_tree_bwd(const harp_tree_model* m, const float* in_pose, const float* betas, const float* transl, int B, float* ws,
                      float* g_verts, const float* g_joints, float* g_in_pose, float* g_betas, float* g_transl, hipStream_t stream);

/* ---- fused per-frame mesh chain -----------------------------------------------------------------------------------
 * One launch (one 1024-thread workgroup per frame, the frame's mesh staged in LDS) for everything utils/visualize.py:45-64
 * (prepare_mesh: /1000, SubdivideMeshes, verts_normals, displacement), Meshes.verts_normals_packed of the displaced mesh
 * (renderer_helper.py:495), hand_verts.mean(1) + process_info_for_shadow (optimize_sequence.py:476, renderer_helper.py:454-468) and
 * MeshRasterizer.transform of both views do between the hand layer and the rasterisers — and one launch for their autograd.
 * Same arithmetic as harp_subdivide_* / harp_vertex_normals_* / harp_displace_bwd / harp_centroid / harp_light_setup_* /
 * harp_project_*; exists because every kernel node of a captured step costs ~4.5 us of dispatch latency.  V0 + E0 <=
 * harp_mesh_chain_max_vertices(), NJ * 3 <= 1024.  PRECONDITION: every vertex of the (subdivided) mesh lies in at least one face
 * (vf_off[i + 1] > vf_off[i] for all i): the kernels pre-fetch vf_tri[vf_off[i] + min(q, n - 1)], which for a vertex in no face
 * reads one entry before its range.  All pointers device memory; "(+=)" outputs accumulate. */
typedef struct harp_mesh_chain {
  const int32_t* edges0;    /* (E0,2) base-mesh edges (midpoint i = V0 + i) */
  const int32_t* vf_off;    /* (V+1) vertex -> incident (face, corner) CSR offsets */
  const int32_t* vf_tri;    /* (nnz,4) per CSR entry: the incident face's vertex ids i0, i1, i2 and this vertex's corner (16-B aligned) */
  const int32_t* sub_off;   /* (V0+1) base vertex -> midpoint CSR (backward) */
  const int32_t* sub_idx;
  const float* disp;        /* (V,) verts_disps */
  int B, V0, E0, NJ, S;
  float focal;
  int shadow;               /* light-view outputs / gradients wanted */
  int has_normal_grad;      /* backward: g_n2 is given (appearance stage) */
  int light_only;           /* backward: ONLY the light-view part — projection backward of g_ndc_l, light camera backward -> g_light_pos (+=);
                             * everything else (camera view, both normal passes, displacement, subdivision, g_v0 / g_joints_mm / g_cam_T /
                             * g_disp) is left out and not written.  The appearance-only stage of a fit: its optimiser holds no geometry
                             * (optimize_sequence.py:264-310), the light position is the one parameter of it this chain feeds. */
  /* forward in */
  const float* verts_mm;    /* (B,V0,3) hand-layer vertices, millimetres */
  const float* joints_mm;   /* (B,NJ,3) */
  const float* cam_R;       /* (B,9) */
  const float* cam_T;       /* (B,3) */
  const float* light_pos;   /* (B,3) */
  /* forward out (backward in) */
  float* joints_m;          /* (B,NJ,3) */
  float* vs;                /* (B,V,3) subdivided, metres */
  float* n1;                /* (B,V,3) its unit vertex normals */
  float* il1;               /* (B,V) 1/|N| (0 where clamped) */
  float* vd;                /* (B,V,3) displaced */
  float* n2;                /* (B,V,3) */
  float* il2;               /* (B,V) */
  float* ndc_c;             /* (B,V,3) camera view */
  float* centroid;          /* (B,3)   shadow only */
  float* light_R;           /* (B,9)   shadow only */
  float* light_T;           /* (B,3)   shadow only */
  float* ndc_l;             /* (B,V,3) shadow only */
  /* backward in */
  const float* g_ndc_c;     /* (B,V,3) */
  const float* g_ndc_l;     /* (B,V,3) shadow only */
  const float* g_n2;        /* (B,V,3) if has_normal_grad */
  const float* g_joints_m;  /* (B,NJ,3) */
  const float* g_vd;        /* (B,V,3) gradient w.r.t. the displaced vertices gathered so far (mesh regularisers, shader) */
  const float* g_light_R;   /* (B,9)  the shader's share, shadow only */
  const float* g_light_T;   /* (B,3) */
  /* backward out */
  float* g_v0;              /* (B,V0,3) w.r.t. verts_mm */
  float* g_joints_mm;       /* (B,NJ,3) */
  float* g_light_pos;       /* (B,3) (+=) shadow only */
  float* g_cam_T;           /* (B,3) (+=) */
  float* g_disp;            /* (V,)  (+=, atomics over frames) */
} harp_mesh_chain;
int harp_mesh_chain_max_vertices(void);
int harp_mesh_chain_fwd(const harp_mesh_chain* a, hipStream_t stream);
int harp_mesh_chain_bwd(const harp_mesh_chain* a, hipStream_t stream);
/* The same forward chain on FOUR workgroups per frame (csrc/chain_wide.hip): each owns a contiguous quarter of the vertices (one per thread),
 * stages the whole frame's positions in LDS, and the two points where a part needs the others' results (displaced neighbours, centroid) are
 * kernel boundaries — two launches of 4 B workgroups instead of one of B.  Same outputs as harp_mesh_chain_fwd (the centroid is the sum of
 * four partial sums).  clear_grads != 0: a->g_vd / a->g_joints_m are zeroed (harp_step_frame.clear_mesh_grads).
 * part_ws: harp_mesh_chain_wide_ws_floats(B, V0 + E0) floats of scratch (shared with harp_mesh_chain_bwd_wide).  (V0 + E0) / 4 <= 1024 and (V0 + E0) * 12 B <= 64 KB. */
size_t harp_mesh_chain_wide_ws_floats(int B, int V);
int harp_mesh_chain_fwd_wide(const harp_mesh_chain* a, int clear_grads, float* part_ws, hipStream_t stream);
/* harp_mesh_chain_bwd on four workgroups per frame: projections backward + normal-length backward | normal gather + displacement |
 * normal gather | SubdivideMeshes backward — four launches, the same outputs (camera sums are sums of four partial sums).  Not for
 * a->light_only (HARP_ERR_ARG: that variant is one small pass of harp_mesh_chain_bwd).  (V0 + E0) * 24 B of LDS per workgroup. */
int harp_mesh_chain_bwd_wide(const harp_mesh_chain* a, float* part_ws, hipStream_t stream);

/* ---- losses, texture helpers, optimiser ---------------------------------------------------------------------------
 * Every loss call accumulates (+=) its value into `loss` and, if `w` (device pointer to the weight(s) = d total/d term)
 * and the gradient output are non-NULL, its weighted gradient (+= unless noted).  Sizes (B, n, n_per_frame, C, H, W) <= 0 return
 * HARP_ERR_ARG without launching, as do n == 0 for harp_adam_step and n_per_frame not a multiple of C for harp_image_l1. */
/* torch.nn.L1Loss between pred*mask and target[fid]*mask[fid] (optimize_sequence.py:519, 543); g_pred is overwritten */
int harp_image_l1(const float* pred, const float* target, const float* mask, const int32_t* fid, int B, int n_per_frame, int C,
                  const float* w, float* loss, float* g_pred, hipStream_t stream);
/* kps_loss (loss/kps_loss.py:4-17); gt (T,21,3) mm indexed by fid, pred (B,n_joints_pred,3) m */
int harp_kps_loss(const float* gt, const int32_t* fid, const float* pred, int B, int n_joints_pred, const float* w, float* loss,
                  float* g_pred, hipStream_t stream);
/* loss[0..2], w[0..2] = mesh_laplacian_smoothing, mesh_normal_consistency (optimize_sequence.py:536-537),
 * arap_loss (loss/arap.py:4-57; ref_verts (V,3), NULL skips it and leaves loss[2] untouched); nbr_*: vertex->neighbour CSR (= the edge
 * list, E edges), nc_pairs (P,4) [v0,v1,a,b] per face pair sharing edge (v0,v1), vp_*: vertex -> (pair*4+role) CSR (harp_amd/topology.py).
 * loss[0..2] and g_verts (B,V,3) accumulate; w or g_verts NULL: the losses only, g_verts untouched.  A vertex of degree 0 has the
 * Laplacian row -v (1/deg taken as 0, as PyTorch3D's laplacian_packed does); P = 0 gives a normal-consistency loss of 0.  B <= 0,
 * V <= 0, P < 0 or E < 0 return HARP_ERR_ARG without launching (harp_mesh_kps_terms likewise). */
int harp_mesh_regularizers(const float* verts, const float* ref_verts, const int32_t* nbr_off, const int32_t* nbr_idx,
                           const int32_t* nc_pairs, const int32_t* vp_off, const int32_t* vp_idx, int B, int V, int P, int E,
                           const float* w, float* loss, float* g_verts, hipStream_t stream);
/* harp_mesh_regularizers + harp_kps_loss (kps_gt, fid, kps_pred, n_joints_pred, w_kps, loss_kps, g_kps_pred as there) in ONE launch:
 * both run between the hand layer and the backward pass of a fitting step and depend on nothing else (optimize_sequence.py:523-537) */
int harp_mesh_kps_terms(const float* verts, const float* ref_verts, const int32_t* nbr_off, const int32_t* nbr_idx,
                        const int32_t* nc_pairs, const int32_t* vp_off, const int32_t* vp_idx, int B, int V, int P, int E,
                        const float* w, float* loss, float* g_verts, const float* kps_gt, const int32_t* fid, const float* kps_pred,
                        int n_joints_pred, const float* w_kps, float* loss_kps, float* g_kps_pred, hipStream_t stream);
/* torch.sum(verts_disps ** 2) (optimize_sequence.py:533) */
int harp_sum_squares(const float* x, int n, const float* w, float* loss, float* g, hipStream_t stream);
/* torch.nn.MSELoss()(x, y) over n elements, ACCUMULATED into *loss (zero it first), and d/dx written to g_x (may be NULL): the
 * objective of the MANO-to-METRO vertex fit (metro_modifications/hand_utils.py:71, 80, 100) */
int harp_mse(const float* x, const float* y, int n, float* loss, float* g_x, hipStream_t stream);
/* albedo_reg / smooth_texture_reg (loss/texture_reg.py:5-30, 48-66) with the drawn integer offsets dist (H,W,2) */
int harp_texture_smooth_reg(const float* tex, const int32_t* dist, const float* mask, int H, int W, const float* w, float* loss,
                            float* g_tex, hipStream_t stream);
/* draws dist (H,W,2) = int(N(0,std)) like torch.normal(...).to(torch.int) at loss/texture_reg.py:15, 51, from a counter-based generator
 * (same values on every rank for the same seed) and, if dist2 != NULL, an independent second set with std2 in the same launch.
 * *counter_dev (one int, device memory) is advanced on the device after the draw, so graph replays draw fresh offsets. */
int harp_draw_texture_offsets(unsigned seed, int* counter_dev, int H, int W, float std, int32_t* dist, float std2, int32_t* dist2,
                              hipStream_t stream);
/* The parameter-only regularisers of a step in ONE launch (optimize_sequence.py:533, 549-551): harp_texture_smooth_reg(tex, dist_albedo)
 * -> loss_albedo / g_tex, harp_close_to_z_reg(nmap, z_scale) + harp_texture_smooth_reg(nmap, dist_normal) -> loss_normal / g_nmap (one
 * weight, as the reference adds the two into one term), and — when disp != NULL — harp_sum_squares(disp, n_disp) -> loss_disp / g_disp.
 * Same per-element arithmetic as the stand-alone calls; the gradient images are accumulated with atomics.  draw_counter_bump (optional):
 * *draw_counter_bump += 1 — the counter harp_step_prologue drew dist_albedo / dist_normal for, advanced by the launch that consumes them. */
int harp_texture_terms(const float* tex, const float* nmap, const float* mask, const int32_t* dist_albedo, const int32_t* dist_normal,
                       int H, int W, float z_scale, const float* w_albedo, float* loss_albedo, float* g_tex, const float* w_normal,
                       float* loss_normal, float* g_nmap, const float* disp, int n_disp, const float* w_disp, float* loss_disp,
                       float* g_disp, int* draw_counter_bump, hipStream_t stream);
/* scale * close_to_z_reg (loss/texture_reg.py:40-45) */
int harp_close_to_z_reg(const float* nm, int H, int W, float scale, const float* w, float* loss, float* g_nm, hipStream_t stream);
/* F.normalize(normal_map, dim=-1) (utils/visualize.py:99); n = number of texels */
int harp_normalize3_fwd(const float* x, int n, float* y, hipStream_t stream);
int harp_normalize3_bwd(const float* x, const float* gy, int n, float* gx, hipStream_t stream);
/* torch.optim.Adam step on a flat fp32 segment (optimize_sequence.py:265-310, 567-573); grad is read as g*grad_scale */
int harp_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps, int step,
                   float grad_scale, hipStream_t stream);

/* graph-replayable variant: hyper-parameters live in device memory (the host updates lr between epochs, e.g. for
 * ReduceLROnPlateau, optimize_sequence.py:309, 581-582); harp_adam_tick advances `step` and the bias corrections. */
typedef struct harp_adam_hyper {
  float lr, beta1, beta2, eps, grad_scale;
  int step;
  float step_size, inv_sqrt_bc2;   /* derived by harp_adam_tick */
} harp_adam_hyper;
int harp_adam_tick(harp_adam_hyper* h_dev, int count, hipStream_t stream);   /* `count` consecutive structs (one per param group) */
int harp_adam_apply(float* p, const float* g, float* m, float* v, size_t n, const harp_adam_hyper* h_dev, hipStream_t stream);
/* both optimisers of a stage (opt_coarse + opt_app, optimize_sequence.py:567-573) in one launch: elements [o0, o0+n0) of the four
 * arenas step with h2_dev[0], elements [o1, o1+n1) with h2_dev[1] */
int harp_adam_apply2(float* p, const float* g, float* m, float* v, size_t o0, size_t n0, size_t o1, size_t n1,
                     const harp_adam_hyper* h2_dev, hipStream_t stream);
/* The head of a fitting step's parameter-only work in ONE launch (any part optional): zero[0..n_zero) = 0 (the step's gradient slab),
 * harp_adam_tick(hyper, n_hyper), and the draw of harp_draw_texture_offsets for the CURRENT value of *draw_counter — which is NOT
 * advanced here (harp_step_frame.draw_counter: the epilogue of the same step advances it). */
int harp_step_prologue(float* zero, size_t n_zero, harp_adam_hyper* hyper_dev, int n_hyper, unsigned seed, const int* draw_counter,
                       int H, int W, float std, int32_t* dist, float std2, int32_t* dist2, hipStream_t stream);

/* ---- per-frame glue of the fitting loop ---------------------------------------------------------------------------
 * replaces the row gathers params[k][fid] of utils/visualize.py:26-27,38-39 / optimize_sequence.py:464, the camera
 * convention of utils/visualize.py:268-271, optimize_sequence.py:453-456 (shared light), :478-480 + renderer_helper.py:
 * 435-441 (ambient ratio -> light colours) and process_info_for_shadow (renderer_helper.py:454-468).
 * The tables are the reference's parameter dict (optimize_sequence.py:181-250) laid out in one flat fp32 arena.
 * B <= 0 returns HARP_ERR_ARG without launching (harp_frame_setup_fwd / _bwd, harp_light_setup_fwd / _bwd), as the sizes of the loss calls. */
typedef struct harp_frame_tables {
  const float *pose, *rot, *trans, *cam;   /* (T,45) (T,3) (T,3) (T,3) */
  const float *shape;                      /* (10,) */
  const float *light_positions;            /* (T,3) */
  const float *amb_ratio;                  /* (1,) pre-sigmoid */
  float *g_pose, *g_rot, *g_trans, *g_cam, *g_shape, *g_light_positions, *g_amb_ratio;   /* gradient arena (+=), NULL = skip */
  int share_light;                         /* configs["share_light_position"] */
  /* SMPL-X arm path (use_arm): pose rows become [rot(3), wrist_pose(3), pose(45)] and betas are padded with zeros to n_betas_out */
  const float *wrist_pose;                 /* (T,3) or NULL (MANO path: rows are [rot(3), pose(45)]) */
  float *g_wrist_pose;
  int n_betas_out;                         /* 10 (MANO) or 20 (SMPL-X: 10 betas + 10 zero expression coefficients) */
} harp_frame_tables;
int harp_frame_setup_fwd(const harp_frame_tables* t, const int32_t* fid, int B, int S, float focal, int self_shadow, float* pose48,
                         float* betas, float* trans_b, float* cam_R, float* cam_T, float* light_pos, float* colors,
                         hipStream_t stream);
int harp_frame_setup_bwd(const harp_frame_tables* t, const int32_t* fid, int B, int S, float focal, int self_shadow,
                         const float* g_pose48, const float* g_betas, const float* g_trans_b, const float* g_cam_T,
                         const float* g_light_pos, const float* g_colors, hipStream_t stream);

/* ---- fused per-frame front of a fitting step, MANO path (csrc/hand_front.hip) ------------------------------------------
 * ONE launch = harp_frame_setup_fwd + harp_lbs_mano_fwd + harp_mesh_chain_fwd.  chain.verts_mm / chain.joints_mm are OUTPUTS
 * here; chain.cam_R / cam_T / light_pos must alias cam_R / cam_T / light_pos below (written by this call).  tables.wrist_pose
 * must be NULL (MANO rows), chain.V0 = 778, chain.NJ = 21. */
/* Optional book-keeping of a fitting step carried by the two per-frame launches instead of kernels of their own (all NULL / 0: none).
 * Front (harp_hand_front_fwd): with `schedule` set, workgroup b takes its frame from row (sched_row[0] mod n_rows) of the (n_rows,B)
 * device schedule and WRITES it to fid[b] (fid is then an output) and fid - target_offset to tfid_out[b] — the DataLoader's batch
 * (optimize_sequence.py:396-399, :446), what harp_schedule_next does as a launch; clear_mesh_grads: chain.g_vd / chain.g_joints_m of
 * the frame are zeroed (the two gradient segments the key-point / mesh terms accumulate into).
 * Back (harp_hand_back_bwd; every kernel that adds to the loss vector has finished by then): sched_row[0] = row + 1;
 * loss_out[0..n_loss) = loss[0..n_loss) and loss[..] = 0 (the terms of the NEXT step accumulate into a clean vector, no clear at the
 * head of a step), loss_total[0] += loss_w . loss when both are given; draw_counter[0] += 1 (harp_draw_texture_offsets_at of the next step draws fresh offsets). */
typedef struct harp_step_frame {
  const int32_t* schedule;
  const int32_t* tschedule;   /* optional (n_rows,B): rows of the resident targets (a dataset that holds a subset / another order of the frames);
                               * NULL: tfid = fid - target_offset */
  int32_t* sched_row;
  int n_rows, target_offset;
  int32_t* tfid_out;
  int clear_mesh_grads;
  float* loss;
  float* loss_out;
  int n_loss;
  int32_t* draw_counter;
  const float* loss_w;        /* optional (n_loss,): back: loss_total[0] += sum_k loss_w[k] * loss[k] — the step's sum_loss */
  float* loss_total;          /*   (optimize_sequence.py:553-559) accumulated over an epoch on the device, no per-step host arithmetic */
} harp_step_frame;

typedef struct harp_hand_front {
  harp_mesh_chain chain;
  harp_mano_model mano;
  harp_frame_tables tables;
  const int32_t* fid;        /* (B,) frame of each batch row */
  float *pose48, *betas, *trans_b, *cam_R, *cam_T, *light_pos, *colors;   /* as harp_frame_setup_fwd */
  float* lbs_ws;             /* harp_lbs_mano_ws_floats(B) floats, kept for harp_lbs_mano_bwd */
  int self_shadow;           /* colours from amb_ratio (shadow renderer) or the fixed Phong lights */
  harp_step_frame step;      /* optional prologue / epilogue of a fitting step (zero-initialised: none) */
} harp_hand_front;
int harp_hand_front_fwd(const harp_hand_front* h, hipStream_t stream);
/* harp_hand_front_fwd on four workgroups per frame: the hand layer with a quarter of the 778 vertices per workgroup (every workgroup
 * gathers the rows and runs the 16-joint chain; the frame's 1.35 MB of blend-shape rows go through four CUs' L1) + harp_mesh_chain_fwd_wide:
 * THREE launches of 4 B workgroups.  Same outputs, same `step` semantics.  part_ws as for harp_mesh_chain_fwd_wide. */
int harp_hand_front_wide_fwd(const harp_hand_front* h, float* part_ws, hipStream_t stream);
/* hybrid: the hand layer on four workgroups per frame, then harp_mesh_chain_fwd (one workgroup per frame): two launches, same outputs */
int harp_hand_front_hybrid_fwd(const harp_hand_front* h, hipStream_t stream);
/* The counterpart for the backward tail of a step (csrc/hand_back.hip): harp_mesh_chain_bwd + harp_lbs_mano_bwd + harp_frame_setup_bwd
 * (autograd of utils/visualize.py:16-88 / manopth/manolayer.py:108-296 down to the rows params[...][fid]) as THREE launches instead of
 * six: mesh chain + joint split + per-vertex skinning backward + trans / cam / light scatter per frame, the two vertex reductions, the
 * kinematic chain backward with the pose / rot / shape scatter.  `h` as passed to harp_hand_front_fwd of the same step, with the chain's
 * gradient inputs filled in (g_ndc_c, g_ndc_l, g_vd, g_n2, g_joints_m, g_light_R / g_light_T, has_normal_grad); gradients are ADDED to
 * the rows tables.g_* (pose, rot, trans, cam, shape and — when g_colors is given, i.e. an appearance stage ran — light_positions,
 * amb_ratio).  g_colors: 9 floats (dL/d colours) or NULL; g_betas_scratch: B*10 floats of scratch. */
int harp_hand_back_bwd(const harp_hand_front* h, const float* g_colors, float* g_betas_scratch, hipStream_t stream);
/* harp_hand_back_bwd with the mesh-chain backward (harp_mesh_chain_bwd_wide's first three launches) and the per-vertex hand-layer backward on
 * four workgroups per frame: SIX launches of mostly 4 B workgroups instead of three of B.  Same results to float32 summation order;
 * chain.light_only is forwarded to harp_hand_back_bwd.  part_ws as for harp_mesh_chain_fwd_wide. */
int harp_hand_back_wide_bwd(const harp_hand_front* h, const float* g_colors, float* g_betas_scratch, float* part_ws, hipStream_t stream);

/* ---- fused per-frame front / back of a fitting step, SMPL-X arm path (csrc/arm_front.hip) ---------------------------------
 * replaces, for configs["use_arm"], what harp_hand_front_fwd / harp_hand_back_bwd replace for the MANO hand: the row gathers
 * params[...][fid] (utils/visualize.py:26-27, 37-40), SMPLXARM.forward(..., return_type='mano_w_arm') (hand_models_harp/
 * body_models.py:2163-2390) and prepare_mesh (utils/visualize.py:45-64) with both projections and the light camera
 * (renderer_helper.py:344, 353, 454-468) — and their autograd down to the gradient rows of the parameter tables.
 * Front = THREE launches: harp_frame_setup_fwd + joint chain per frame | the blend-shape contraction of all frames on the matrix
 * cores | skinning + output joints + harp_mesh_chain_fwd per frame.  Back = FOUR: harp_mesh_chain_bwd + joint split + recentring
 * + skinning backward + trans / cam / light / ambient scatter per frame | the two vertex reductions (MFMA) | the kinematic chain
 * backward with the rot / wrist_pose / pose / shape scatter.  Same arithmetic as harp_frame_setup_* + harp_lbs_tree_* +
 * harp_mesh_chain_*; `step` as in harp_hand_front.  tables.wrist_pose must be set (rows [rot, wrist_pose, pose] = 51 floats),
 * tables.n_betas_out = tree.NB, chain.V0 = tree.NV, chain.NJ = tree.n_joints_out; chain.verts_mm / joints_mm are OUTPUTS;
 * chain.cam_R / cam_T / light_pos must alias cam_R / cam_T / light_pos below. */
typedef struct harp_arm_front {
  harp_mesh_chain chain;
  harp_tree_model tree;
  harp_frame_tables tables;
  const int32_t* fid;        /* (B,) frame of each batch row */
  float *pose_in, *betas, *trans_b, *cam_R, *cam_T, *light_pos, *colors;   /* as harp_frame_setup_fwd: (B,51) (B,NB) (B,3) (B,9) (B,3) (B,3) (9) */
  float* lbs_ws;             /* harp_lbs_tree_ws_floats(&tree, B) floats, shared by the front and the back of one step */
  const float* weights_T;    /* (NJ, NV): tree.weights transposed (the per-frame kernels read one coalesced row per joint) */
  int self_shadow;           /* colours from amb_ratio (shadow renderer) or the fixed Phong lights */
  harp_step_frame step;      /* optional prologue / epilogue of a fitting step (zero-initialised: none) */
} harp_arm_front;
int harp_arm_front_fwd(const harp_arm_front* h, hipStream_t stream);
/* `h` as passed to harp_arm_front_fwd of the same step, with the chain's gradient inputs filled in (see harp_hand_back_bwd); gradients
 * are ADDED to the rows tables.g_* (pose, rot, wrist_pose, trans, cam, shape and — when g_colors is given — light_positions, amb_ratio).
 * g_pose_scratch: B*51 floats (holds dL/d pose rows afterwards), g_betas_scratch: B*NB floats. */
int harp_arm_back_bwd(const harp_arm_front* h, const float* g_colors, float* g_pose_scratch, float* g_betas_scratch, hipStream_t stream);
/* The same front / back with the per-frame work on FOUR workgroups per frame around harp_mesh_chain_fwd_wide / _bwd_wide
 * (a quarter of the vertices per workgroup; 5 + 7 launches).  part_ws: harp_mesh_chain_wide_ws_floats(B, V0 + E0) floats.
 * chain.light_only is forwarded to harp_arm_back_bwd. */
int harp_arm_front_wide_fwd(const harp_arm_front* h, float* part_ws, hipStream_t stream);
int harp_arm_back_wide_bwd(const harp_arm_front* h, const float* g_colors, float* g_pose_scratch, float* g_betas_scratch, float* part_ws,
                           hipStream_t stream);

int harp_light_setup_fwd(const float* centroid, const float* light_pos, int B, float* light_R, float* light_T, hipStream_t stream);
int harp_light_setup_bwd(const float* centroid, const float* light_pos, const float* g_light_R, const float* g_light_T, int B, int V,
                         float* g_light_pos, float* g_centroid, float* g_verts, hipStream_t stream);
/* y = s * x over n floats (n <= 0: HARP_ERR_ARG, no launch) */
int harp_scale(const float* x, float s, int n, float* y, hipStream_t stream);
/* replaces the DataLoader's batch of frame ids (optimize_sequence.py:396-399, :446): row (counter[0] mod n_rows) of a device-resident
 * (n_rows,B) int32 schedule -> fid (B,), tfid = fid - target_offset; then counter[0] = row + 1.  Graph-replayable. */
int harp_schedule_next(const int32_t* schedule, int n_rows, int B, int target_offset, int32_t* counter, int32_t* fid, int32_t* tfid,
                       float* zero, int n_zero, hipStream_t stream);   /* zero (optional): n_zero floats cleared in the same launch (loss vector) */
/* the same with the target rows given by a second (n_rows,B) table instead of fid - target_offset (tschedule == NULL: as above) */
int harp_schedule_next_rows(const int32_t* schedule, const int32_t* tschedule, int n_rows, int B, int target_offset, int32_t* counter,
                            int32_t* fid, int32_t* tfid, float* zero, int n_zero, hipStream_t stream);

/* ---- perceptual term: 3x3 convolutions on the matrix cores ----------------------------------------------------------------------------
 * replaces the torch.nn.Conv2d / ReLU / MaxPool2d stack of model/vgg.py:10-56 (torchvision vgg16.features[0:23]; built at
 * optimize_sequence.py:405, evaluated on y_pred * mask and y_true * mask at :546-547, weight 1.0 at :419) and its autograd: F.conv2d
 * (cuDNN in the reference), threshold_backward, max_pool2d_with_indices_backward, L1Loss.  The filters are frozen (requires_grad=False,
 * model/vgg.py:34-36): only data gradients exist.
 * Activations are NHWC float32.  harp_conv3x3 is one 3x3 / pad 1 / stride 1 convolution (Cin % 16 == 0, Cout % 64 == 0; pad the
 * channels with zeros otherwise) with one of four fused epilogues:
 *   HARP_CONV_RELU      out = relu(conv + bias); pooled (optional, H and W even) = max_pool2d(out, 2, 2); out may be NULL when pooled is not
 *   HARP_CONV_RELU_TAP  the same, plus the tap's share of L1Loss(features(pred), features(target)): *loss (+=, double) tap_scale * sum|out - target|,
 *                       g_tap = tap_scale * sign(out - target) * [out > 0]  (d loss / d conv, ReLU backward applied);
 *                       target (T,H,W,Cout) row target_row[n] (NULL: row n)
 *   HARP_CONV_GATE      data gradient through the ReLU in front of this convolution's input: out = conv * [gate > 0], gate (N,H,W,Cout)
 *   HARP_CONV_UNPOOL    data gradient through max pool + ReLU: the convolution runs at the pooled size (H,W); out and gate are (N,2H,2W,Cout);
 *                       out (+=) the result routed to the first maximum of each 2x2 window of gate where that maximum is positive
 * precision HARP_CONV_F32 (0): v_mfma_f32_32x32x2_f32 (float32 fma chain); HARP_CONV_BF16X3 (1): three-term bf16 split, float32 accumulate
 * (~16 mantissa bits per product); HARP_CONV_F16 (2): one v_mfma_f32_32x32x16_f16 product per MAC, float32 accumulate — both operands
 * rounded to f16 (11-bit significand, round to nearest even), the precision class of TF32.  f16's range is moved per launch: the input is
 * staged as f16(in * 2^e) and the float32 accumulator is multiplied by 2^-e before the epilogue (a power of two: no rounding changes,
 * values are only kept in f16's normal range), with e = in_exp - floor(log2(*in_amax)) when in_amax != NULL (an upper bound of |in| on the
 * device: in_exp = 14 stages the largest value in [2^14, 2^15)), else e = in_exp; e is clamped to [-126, 126].  Every f32 -> f16
 * conversion (activations and filters) saturates at +-65504, never inf.  Filters of magnitude below 6.1e-5 keep an absolute error of 3e-8.
 * filters: harp_conv3x3_pack_filters output for the same precision (transpose = 1 packs the data-gradient filters of a forward (Cout,Cin,3,3)
 * weight: channels swap roles, taps are mirrored). */
#define HARP_CONV_F32 0
#define HARP_CONV_BF16X3 1
#define HARP_CONV_F16 2
#define HARP_CONV_RELU 0
#define HARP_CONV_RELU_TAP 1
#define HARP_CONV_GATE 2
#define HARP_CONV_UNPOOL 3
typedef struct harp_conv3x3_args {
  const float* in;            /* (N,H,W,Cin) */
  const void* filters;        /* harp_conv3x3_filter_bytes(Cout,Cin) bytes */
  const float* bias;          /* (Cout) or NULL */
  float* out;
  float* pooled;              /* (N,H/2,W/2,Cout) or NULL */
  const float* target;
  const int32_t* target_row;
  float* g_tap;
  double* loss;
  const float* gate;
  int N, H, W, Cin, Cout;
  int precision, epilogue;
  int in_channels;            /* channels per pixel of `in` in memory (multiple of 4, <= Cin; the rest reads as zero); 0 = Cin */
  float tap_scale;
  /* bounded mode (all NULL / 0 = every tile): image n belongs to frame row r = target_row[n]; only the 16x16 output tiles of that frame's
   * list are computed, and input pixels in cells this pass did not write are taken from in_alt (the same activation of another pass,
   * e.g. the target frame's, rows through target_row) or read as zero.  Everything outside the listed tiles is left as it was: `out`, `pooled` (a 2x2
   * window belongs to the tile of its pixels) and g_tap; *loss receives the listed tiles' share only.  tile_list, tile_origin, in_valid, in_alt, out_valid
   * and their origins are all indexed by the frame row r.  Origins are non-negative; list entries past tile_count[r] are not read */
  const int32_t* tile_list;   /* (T, max_tiles): ty * tile_pitch + tx in the frame's tile grid */
  const int32_t* tile_count;  /* (T) */
  int max_tiles;
  int in_valid_shift;         /* cells of in_valid are (8 << shift) input pixels square: 1 = the producer's 16x16 tiles, 0 = tiles of a 2x finer producer behind a pool */
  const int32_t* in_valid;    /* (T, in_valid_pitch^2) 0/1 over the PRODUCER's tile grid; a cell at or beyond in_valid_pitch (in y or in x) counts as not written */
  const float* in_alt;        /* (T,H,W,in_channels) or NULL: zero */
  const int32_t* out_valid;   /* HARP_CONV_UNPOOL: (T, out_valid_pitch^2) 0/1 over the tile grid of `out` (twice this convolution's resolution); windows elsewhere are skipped */
  /* a frame's tile grid may be shifted so that its tiles hug the active region: tile (ty, tx) covers pixels [16 ty - oy, 16 ty - oy + 16) x
   * [16 tx - ox, ...), origin (oy, ox) EVEN (2x2 pool windows stay inside a tile), per frame, in the pixels of the grid's own resolution;
   * NULL = (0, 0).  pitch = tiles per row (and rows) of the grid's bitmap */
  const int32_t* tile_origin;       /* (T,2) of the grid tile_list indexes */
  const int32_t* in_valid_origin;   /* (T,2) of the producer's grid, in the PRODUCER's pixels: behind a pool (in_valid_shift 0) those are twice as fine as this
                                     * convolution's input pixels and the origin is halved — input pixel (y, x) lies in cell ((y + oy / 2) / cell, (x + ox / 2) / cell) */
  const int32_t* out_valid_origin;  /* (T,2) of `out`'s grid: the window of pooled pixel (y, x) lies in cell ((2 y + oy) / out_valid_cell, (2 x + ox) / out_valid_cell),
                                     * which must exist — the bitmap has to cover `out` (out_valid_pitch is not checked against it) */
  int tile_pitch, in_valid_pitch, out_valid_pitch;
  /* tiles of 8x8 pixels (the coarse levels of the perceptual term, where a hand is a few tiles across): tile_side = 8 — tile_list / tile_origin /
   * tile_pitch then describe a grid of 8-pixel tiles and a workgroup computes four of them (one per wave); 0 or 16 = the 16x16 form.
   * in_valid_cell: side of in_valid's cells in INPUT pixels when the producer's tiles are not 16 pixels (4 — only with tile_side 8 —, 8, 16;
   * 0 = 8 << in_valid_shift; in_valid_shift still says whether the producer sits behind a pool).  out_valid_cell: side of `out`'s tiles (8 or 16; 0 = 16). */
  int tile_side, in_valid_cell, out_valid_cell;
  /* HARP_CONV_F16 only (ignored otherwise): the exponent shift e of the staged input, see above.  NULL / 0 = unscaled */
  const float* in_amax;
  int in_exp;
} harp_conv3x3_args;
size_t harp_conv3x3_filter_bytes(int Cout, int Cin);
int harp_conv3x3_pack_filters(const float* w, int Cout, int Cin, int transpose, int precision, void* packed, hipStream_t stream);
int harp_conv3x3(const harp_conv3x3_args* a, hipStream_t stream);

/* The whole term (optimize_sequence.py:546-547): loss = L1Loss(vgg(y_pred * mask), vgg(y_true * mask)) with vgg = model/vgg.py's
 * Vgg16Features (rows: the image itself, relu1_2, relu2_2, relu3_3, relu4_3, scaled by layers_weights, :51-55), and d loss / d y_pred.
 * harp_vgg16: the ten convolutions in the order of torchvision vgg16.features[0:23] (0, 2, 5, 7, 10, 12, 14, 17, 19, 21): filters[k] /
 * filters_t[k] = harp_conv3x3_pack_filters(w_k, transpose = 0 / 1) for `precision` (the first layer's 3 input channels padded to 16;
 * filters_t[0] unused), bias[k], w0t (9,3,64) = the first layer's data-gradient filters for the vector-ALU kernel that ends the
 * backward pass: w0t[t][c][co] = w0[co][c][8 - t] with w0 the (64,3,3,3) weight, taps flattened.
 * ws: harp_vgg16_ws_bytes(N,S,with_gradient) bytes (S % 8 == 0), zero-filled once by the caller before the first use.
 * harp_vgg16_features: activations of image[rows[n]] * mask[rows[n]] (rows NULL: n), NHWC, into the caller's arrays — its cache of the
 *   target frames' features (they do not change during a fit): out[k], k = 0..9 = relu(convolution k) (N, S/d_k, S/d_k, Cout_k) with
 *   d = 1,1,2,2,4,4,4,8,8,8; out[10..12] = the three pooled maps (N,S/2,S/2,64), (N,S/4,S/4,128), (N,S/8,S/8,256).  The four taps
 *   out[1], out[3], out[6], out[9] (relu1_2 ... relu4_3) are required, the others may be NULL (kept in ws only).
 * Bounded mode of harp_vgg16_term (tiles[0] != NULL; needs target_by_row and the cache of ALL activations): the stack runs only in the
 *   tiles (tile_side[L]: 16 pixels a side, or 8) of each resolution level (L = 0..3, side S >> L) where the rendered image's activations can differ from the target
 *   frame's — tiles[L] (T, tile_pitch[L]^2) 0/1 per frame over a tile grid shifted by the frame's tile_origin[L] (so that the tiles hug the
 *   active region), tile_list[L] (T, max_tiles[L]) their indices, tile_count[L] (T): the support
 *   of mask grown by the receptive field (the caller's set-up, harp_amd/model/vgg_hip.py).  Elsewhere pred == target exactly: the L1
 *   and its gradient vanish, and inputs needed from there are read from target_in[k] = the target frame's input activation of
 *   convolution k (k = 1..9: out[0], out[10], out[2], out[11], out[4], out[5], out[12], out[7], out[8] of harp_vgg16_features).  Same
 *   loss and gradient as the full pass, bit for bit in the tiles it computes.
 * harp_vgg16_term: forward over rgb * mask[rows[n]] with the L1 against target[k] fused into the tap layers, backward to the image:
 *   *loss = the term (unweighted);  g_rgb (N,S,S,3) = covered < 0 ? 0 : g_rgb + weight * d loss / d rgb   (covered NULL: everywhere).
 * precision HARP_CONV_F16: the two entry points choose the exponent shifts themselves — the forward convolutions from max|image * mask| of
 *   the pass (folded on the device: its largest value staged in [1, 2)), the backward ones from the largest tap seed layer_w[k] / n (on the
 *   host: staged in [1, 2)).  Layer weights scaled by 2^k scale the loss and gradient by exactly 2^k. */
typedef struct harp_vgg16 {
  const void* filters[10];
  const void* filters_t[10];
  const float* bias[10];
  const float* w0t;
  float layer_w[5];
  int precision;
} harp_vgg16;
typedef struct harp_vgg16_term_args {
  const float* rgb;            /* (N,S,S,3) rendered images */
  const float* y_true;         /* (T,S,S,3) */
  const float* mask;           /* (T,S,S) */
  const int32_t* rows;         /* (N,) target row of each image; NULL: n */
  const float* target[4];      /* tap features of y_true * mask, layouts of harp_vgg16_features */
  int target_by_row;           /* 1: target[k] holds T rows indexed through `rows`; 0: N rows in batch order */
  const int32_t* covered;      /* (N,S,S) nearest-face ids (< 0: no face) or NULL */
  float* g_rgb;
  float weight;
  float* loss;
  int N, S;
  void* ws;
  const float* target_in[10];
  const int32_t* tiles[4];
  const int32_t* tile_list[4];
  const int32_t* tile_count[4];
  int max_tiles[4];
  const int32_t* tile_origin[4];   /* (T,2) even (oy, ox) per frame and level: tile (ty, tx) covers pixels [16 ty - oy, +16) x [16 tx - ox, +16) */
  int tile_pitch[4];               /* tiles per row (= rows) of tiles[L]; tile_list[L] entries are ty * pitch + tx */
  int tile_side[4];                /* side of level L's tiles in pixels: 16 (0 = 16) or 8; 16 at level 0, and never 16 behind (coarser than) an 8 */
  void* side_streams[3];           /* up to three more hipStream_t (NULL-terminated).  With k of them (and rows, target_by_row) the term runs as k + 1
                                    * parts of the batch, part i > 0 on side_streams[i - 1], forked from and joined back into `stream` by events
                                    * (capturable): the chains of 21 dependent launches fill each other's partly filled last rounds of workgroups.
                                    * Same results. */
} harp_vgg16_term_args;
size_t harp_vgg16_ws_bytes(int N, int S, int with_gradient);
int harp_vgg16_features(const harp_vgg16* net, const float* image, const float* mask, const int32_t* rows, int N, int S, void* ws,
                        float* const* out, hipStream_t stream);
int harp_vgg16_term(const harp_vgg16* net, const harp_vgg16_term_args* t, hipStream_t stream);

/* ---- data-parallel exchange (RCCL over xGMI) -------------------------------------------------------------------------
 * New capability: the reference is single-device.  Frames of a sequence are sharded over the GPUs of a node; between
 * `sum_loss.backward()` and `opt_coarse.step() / opt_app.step()` (optimize_sequence.py:567-573) every rank sums the flat fp32
 * gradient bucket [pose .. normal_map] of the parameter arena in place (1/world is applied by the Adam kernel's grad_scale).
 * RCCL is bound with dlopen at the first harp_comm_* call (the copy an embedding PyTorch process has mapped is reused).
 * harp_comm_unique_id: rank 0 obtains HARP_COMM_ID_BYTES opaque bytes and hands them to every rank over any side channel;
 * harp_comm_create: collective over all ranks, binds the calling thread's current HIP device; the handle is opaque.
 * harp_allreduce_flat only enqueues on `stream` (no host synchronisation), so it can be captured into a hipGraph. */
#define HARP_COMM_ID_BYTES 128
#define HARP_ERR_NO_RCCL 1000
#define HARP_ERR_COMM 1001
int harp_comm_unique_id(void* id_out);
int harp_comm_create(const void* id, int rank, int world, void** comm_out);
int harp_comm_destroy(void* comm);
int harp_allreduce_flat(void* comm, float* buf, size_t n, hipStream_t stream);

/* ---- post-fit evaluation metrics (csrc/metrics.hip) ------------------------------------------------------------------------------
 * replaces utils/eval_util.py:10-60 as called per 64-frame chunk at optimize_sequence.py:713-722: MS_SSIM(data_range=1,
 * size_average=True, channel=3) of pytorch_msssim 0.2.1 (eval_util.py:8, 56-60; ms_ssim / _ssim / gaussian_filter of that package),
 * sil_iou's >= 0.5 mask counts (:41-49) and l1_diff's |ref - pred| sum (:34-38), for N images of C <= 3 channels and H x W pixels.
 * ref / pred: float32 images read in place through element strides (sn, sc, sy, sx) shared by both: the reference's (N,H,W,3) render
 * layout is (H*W*3, 1, W*3, 3), pytorch_msssim's NCHW is (C*H*W, H*W, W, 1).  ref_mask / pred_mask: (N,H,W) contiguous float32, both
 * or neither (NULL: inter = union = 0).  weights: n_levels (1..5) host floats (the package's default [0.0448, 0.2856, 0.3001, 0.2363,
 * 0.1333]); window: 11 taps of a float32 Gaussian of `sigma`; C1 = (K1 * data_range)^2, C2 = (K2 * data_range)^2.
 * out: per image 4 + 2 * n_levels * C floats: inter, union (pixel counts over the full image), l1_sum (over the full image and all
 * channels), ms_ssim (relu, weight powers, channel mean), then ssim[level][channel], then cs[level][channel] (means over each level's
 * valid map).  ws: harp_image_metrics_ws_bytes(N, H, W) bytes, 16-B aligned, no initial contents.  Deterministic: no atomics, fixed
 * reduction order.  Returns HARP_ERR_ARG without launching for NULL images / ws / out / weights, one mask without the other,
 * min(H, W) <= 160 (the package's own assertion (11 - 1) * 2^4), C outside 1..3, n_levels outside 1..5, N outside 1..65535.
 * harp_image_metrics_ws_bytes: pure host arithmetic, 0 for those sizes — with h_0 = H, h_{l+1} = (h_l + 1) / 2 (w likewise),
 * tiles_l = ceil((h_l - 10) / 32) * ceil((w_l - 10) / 32) and A(b) = b rounded up to 256:
 *   sum_{l=1..4} 2 * A(12 * N * h_l * w_l)  +  sum_{l=0..4} A(64 * N * tiles_l). */
size_t harp_image_metrics_ws_bytes(int N, int H, int W);
int harp_image_metrics(const float* ref, const float* pred, const float* ref_mask, const float* pred_mask, long long sn, long long sc,
                       long long sy, long long sx, int N, int C, int H, int W, float data_range, const float* weights, int n_levels,
                       float K1, float K2, float sigma, void* ws, float* out, hipStream_t stream);

/* ---- LPIPS v0.1 / AlexNet of the post-fit evaluation (csrc/lpips.hip) ------------------------------------------------------------
 * replaces lpips.LPIPS(net='alex') as built at utils/eval_util.py:7 and called at :51-53 (lpips_diff, per 64-frame chunk from
 * optimize_sequence.py:737 / :795): version 0.1, lpips=True, spatial=False, eval mode; forward only, float32 (every convolution a float32
 * fma chain on v_mfma_f32_32x32x2_f32).  Scaling layer x' = (x - shift) / scale, shift (-0.030, -0.088, -0.188), scale (0.458, 0.448,
 * 0.450) (normalize != 0: x -> 2x - 1 first; the reference passes [0, 1] images without it); torchvision alexnet.features[0:12] with taps
 * after the five ReLUs; per tap f / (||f||_2 over channels + 1e-10), sum_c lin_k[c] (ref - pred)^2, mean over the tap's H x W.
 * harp_lpips_alex_pack: device float32 weights in torch's layouts — w[k] (Cout,Cin,KS,KS) = (64,3,11,11), (192,64,5,5), (384,192,3,3),
 *   (256,384,3,3), (256,256,3,3); bias[k] (Cout); lin[k] (C_k) = the (1,C_k,1,1) head weights — into `net`, harp_lpips_alex_net_bytes()
 *   bytes, 256-B aligned, opaque (only enqueues: the sources must stay alive until the stream reaches it).
 * harp_lpips_alex: ref / pred (N images, 3 channels, H x W) read in place through element strides (sn, sc, sy, sx) shared by both
 *   (the reference's (N,H,W,3) renders: (3HW, 1, 3W, 3); NCHW: (3HW, HW, W, 1)); both go through the network as one batch of 2N.
 *   out: per image 6 floats: LPIPS, then the five taps' spatial means (relu1 .. relu5; the total is their float64 sum).
 *   ws: harp_lpips_alex_ws_bytes(N, H, W) bytes, 256-B aligned, no initial contents.  Deterministic: no atomics, fixed reduction order;
 *   identical ref and pred give exactly 0.  Returns HARP_ERR_ARG without launching for NULL net / images / ws / out, misaligned net or ws,
 *   min(H, W) < 31 (the second pool's input would be smaller than its window), N outside 1..65535, or a tap map of more than 2^31 / 384
 *   pixels (32-bit offsets inside one image).
 * harp_lpips_alex_ws_bytes: pure host arithmetic, 0 for those sizes — with h1 = (H - 7) / 4 + 1, h2 = (h1 - 3) / 2 + 1, h3 = (h2 - 3) / 2 + 1
 *   (w likewise, integer division), P = 2N, A(b) = b rounded up to 256 and t_k = ceil(h_k w_k / 64) (h_3 = h_4 = h_5 = h3):
 *   A(256 P h1 w1) + A(256 P h2 w2) + A(768 P h2 w2) + A(768 P h3 w3) + A(1536 P h3 w3) + 2 A(1024 P h3 w3)  +  sum_{k=1..5} A(4 N t_k). */
size_t harp_lpips_alex_net_bytes(void);
int harp_lpips_alex_pack(const float* const* w, const float* const* bias, const float* const* lin, void* net, hipStream_t stream);
size_t harp_lpips_alex_ws_bytes(int N, int H, int W);
int harp_lpips_alex(const void* net, const float* ref, const float* pred, long long sn, long long sc, long long sy, long long sx, int N,
                    int H, int W, int normalize, void* ws, float* out, hipStream_t stream);

/* ---- what a fit is looked at with: normal image and uint8 panel strips (csrc/present.hip) -------------------------------------------
 * harp_normal_image replaces MeshRenderer(MeshRasterizer(faces_per_pixel = K, blur_radius = 0), SoftPhongNormalShader) as built at
 * renderer/renderer_helper.py:83-101 and run at :216-301 (called from optimize_sequence.py:710-714 for every frame and from
 * utils/visualize.py:172, 188 for the normal turntable), forward only, in one pass: no (B,S,S,K) fragment buffer is read or written.
 *   ndc (B,V,3) camera-view (x_ndc, y_ndc, z_view) as harp_project_fwd writes them; vnormals (B,V,3); faces (F,3);
 *   ws: harp_rasterize_ws_bytes(B, F, S) bytes, no initial contents (the face set-up of harp_rasterize_fragments_fwd runs first).
 *   Per pixel: the candidates of harp_rasterize_fragments_fwd with blur_radius = 0 (pixel centre inside the face, pz >= 0), the K
 *   nearest by pz kept, ties keep the lower face index; per kept fragment the interpolated vertex normal (perspective-correct
 *   barycentrics, not clipped, not normalised) — with nmap: the bilinear sample (align_corners = True, border padding, v flipped) of the
 *   NORMALISED map at the interpolated uv through PBRMaterials.apply_normal_map (pbr_materials.py:58-124: n' = normalize(-u m.x - v m.y
 *   + n m.z)) — then (x, -y, -z), (. + 1) / 2, and pytorch3d's softmax_rgb_blend(sigma, gamma, znear, zfar, background).
 *   nmap: NULL or (Ht,Wt,3) float32 maps, frame b reading nmap + b * nmap_frame_stride (elements; 0: one shared map), which then needs
 *   verts_uvs (VT,2) and faces_uvs (F,3) (indices are NOT bounds-checked).  background: 3 HOST floats.
 *   out (B,S,S,4) float32: blended rgb, alpha = 1 - prod(1 - prob).  A pixel without a fragment is exactly (background, 0).
 *   Deterministic: no atomics.  Returns HARP_ERR_ARG without launching for NULL ndc / vnormals / faces / background / ws / out,
 *   B outside 1..65535, V, F, S <= 0, K outside 1..16, sigma or gamma <= 0, zfar <= znear, a map without uvs or with Ht, Wt <= 0.
 * harp_panels_u8 replaces the host statement of optimize_sequence.py:744-755 (clip, * 255, concatenate, astype(uint8)) and the
 * clip * 255 -> uint8 of every turntable frame (utils/visualize.py:174-175, 190-191, 222-223): out (N, H, P * W, 3) uint8 with
 * P = n_images + (masks ? 1 : 0) panels side by side.
 *   images: n_images (0..3) HOST pointers to device float32 images, read in place; strides: 4 HOST element strides per image
 *   (image, row, column, channel): an (N,H,W,3) render is (3HW, 3W, 3, 1), the rgb of an (N,H,W,4) normal image (4HW, 4W, 4, 1), NCHW
 *   (3HW, W, 1, HW).  Colour panels: uint8(trunc(clip(x, 0, 1) * 255)), the product in float32 as numpy forms it.
 *   mask_true / mask_pred: both or neither, (N,H,W) contiguous float32; they give the last panel (uint8(trunc(m_true * 225)), 0,
 *   uint8(trunc(m_pred * 225))), the product in float64 as numpy forms it (225 is the reference's factor), saturating outside [0, 255].
 *   Returns HARP_ERR_ARG without launching for NULL out, n_images outside 0..3, a NULL image / strides, a negative stride, one mask without
 *   the other, no panel at all, N, H, W <= 0. */
int harp_normal_image(const float* ndc, const float* vnormals, const int32_t* faces, int B, int V, int F, int S, int K, float sigma, float gamma,
                      float znear, float zfar, const float* background, const float* nmap, long long nmap_frame_stride, int Ht, int Wt,
                      const float* verts_uvs, const int32_t* faces_uvs, void* ws, float* out, hipStream_t stream);
int harp_panels_u8(const float* const* images, const long long* strides, int n_images, const float* mask_true, const float* mask_pred, int N,
                   int H, int W, unsigned char* out, hipStream_t stream);

/* ---- what a running fit is watched with: uint8 contact sheets (csrc/sheet.hip) ---------------------------------------------------------
 * harp_sheet_u8 replaces show_img_pair (optimize_sequence.py:37-64: a 3 x 3 matplotlib figure of the first mini-batch, called at
 * :490-501 every 10 epochs and from visualize_val at :156) and the atlas dumps of visualize_val (:160-168): ONE launch writes one
 * finished sheet out (rows * ch, cols * cw, 3) uint8 of up to rows * cols frames, ch = ceil(H / d), cw = ceil(W / d) for the integer box
 * factor d.  Cell k = r * cols + c shows frame k; cells k >= N are 255 in all channels (an empty axis of the reference's white figure).
 * The cells lie edge to edge (matplotlib's margins and its resampling to a 1000-px figure are not reproduced).
 *   a: (N,H,W[,C]) float32 frames read in place; a_strides: 4 HOST element strides (frame, row, column, channel); b / b_strides likewise;
 *   mask (N,H,W) with 3 HOST strides (frame, row, column).  Colour p of a source pixel, every operation rounded to float32 on its own:
 *     mode 0 IMAGE    p = clip(a[..., 0:3], 0, 1)                                       (:54, :156: imshow clips floats)
 *     mode 1 OVERLAY  p = (clip(a), 0, clip(b)), a = true mask, b = predicted mask; single-channel, the channel strides are ignored (:48-52)
 *     mode 2 ABSDIFF  p = clip(|a * mask - b * mask|) per channel, the two products rounded separately, no fma             (:499-501)
 *     mode 3 NORMAL   p = clip(a / max(|a|, 1e-12) * 0.5 + 0.5)                                                             (:166-167)
 *   clip(x) = fminf(fmaxf(x, 0), 1), so a NaN counts as 0.  Output pixel (i, j) of a cell: v = the sum of p over the source box
 *   y in [i d, min(H, (i + 1) d)), x in [j d, min(W, (j + 1) d)), added by one lane in row-major order from 0.0f, divided (IEEE float32)
 *   by the number of pixels summed; written as uint8(trunc(v * 255.0f)).  d = 1 is harp_panels_u8's colour convention bit for bit.
 *   Stream-ordered and capturable: no allocation, no synchronisation.  Deterministic: no atomics.
 *   Returns HARP_ERR_ARG without launching for mode outside 0..3, NULL a / a_strides / out, N, H, W, rows, cols <= 0, d outside 1..8,
 *   rows * cols > 64, N > rows * cols, a negative stride, a missing operand (modes 1, 2 need b and b_strides, mode 2 needs mask and
 *   mask_strides) and a superfluous one (b in modes 0, 3; mask outside mode 2). */
int harp_sheet_u8(int mode, const float* a, const long long* a_strides, const float* b, const long long* b_strides, const float* mask,
                  const long long* mask_strides, int N, int H, int W, int rows, int cols, int d, unsigned char* out, hipStream_t stream);

/* ---- export of the fitted avatar: Taubin smoothing (csrc/smooth.hip) ----------------------------------------------------------------
 * optimize_sequence.py:780  pytorch3d.ops.taubin_smoothing(meshes, lambd=0.53, mu=-0.53, num_iter=10), forward only (the reference calls
 * it under no_grad).  PyTorch3D is not installed where this was written: the semantics are its v0.6.2 taubin_smoothing / norm_laplacian
 * AS RECALLED, restated here in full.  verts / out (B,V,3) float32; nbr_off (V+1) / nbr_idx the vertex -> neighbour CSR of
 * harp_amd/topology.py, shared by all frames (indices are NOT bounds-checked).  Per frame, num_iter times: one pass with factor lambd, then
 * one with factor mu.  A pass with factor f moves every vertex from the PREVIOUS pass's positions (Jacobi), weights recomputed per pass:
 *   w_ij = 1 / (|v_i - v_j| + 1e-12) for j in nbr(i),   v_i' = (1 - f) v_i + f (sum_j w_ij v_j) / (sum_j w_ij)
 * (evaluated as v_i + f sum_j w_ij (v_j - v_i) / sum_j w_ij).  Deviation: a vertex without neighbours keeps its position (PyTorch3D
 * yields 0/0 = NaN there).  num_iter = 0 copies verts to out bit for bit.  out may alias verts.  Stream-ordered and capturable: no
 * allocation, no synchronisation.  Deterministic: no atomics.
 * mode 1: one workgroup per frame, the positions resident in LDS for all 2 * num_iter passes; V <= 4096 (64 KiB), otherwise HARP_ERR_ARG;
 *   ws is not used.  mode 2: one launch per pass, ping-pong through ws = harp_taubin_ws_bytes(B, V) bytes (256-B aligned, no initial
 *   contents); any V.  mode 0: mode 1 where V fits, else mode 2.
 * Returns HARP_ERR_ARG without launching for NULL verts / nbr_off / nbr_idx / out, B <= 0, V <= 0, num_iter < 0, mode outside 0..2, and a
 * NULL ws where mode 2 runs with num_iter > 0.
 * harp_taubin_ws_bytes: pure host arithmetic, 2 * (12 B V rounded up to 256); 0 for B <= 0 or V <= 0. */
size_t harp_taubin_ws_bytes(int B, int V);
int harp_taubin_smooth(const float* verts, const int32_t* nbr_off, const int32_t* nbr_idx, int B, int V, float lambd, float mu, int num_iter,
                       int mode, float* out, void* ws, hipStream_t stream);

/* ---- geometric accuracy of the post-fit evaluation: Procrustes, PCK counts, point-set F-score (csrc/pose_eval.hip) --------------------
 * All three only enqueue on `stream`: no allocation, no workspace, no synchronisation, capturable.  Forward only, float64 inside, no float
 * atomics and a fixed order in every sum, so a repeated call gives the same bits.
 *
 * harp_procrustes_align replaces align_w_scale (utils/eval_util.py:212-235, with scipy.linalg.orthogonal_procrustes inside) as called
 * once per frame from optimize_sequence.py:760-774 and utils/eval_util.py:199, for N frames in one launch (one workgroup per frame).
 *   gt (N,K,3), pred (N,Kp,3) float32; pred_idx NULL (then Kp must equal K, points in order) or K int32 indices into the Kp points (the
 *   gather `pred[:, right_mano_idx]` without a copy; an index outside [0, Kp) is never read: that point counts as invalid);
 *   valid NULL or (N,K) float32, non-zero = the point is used.  Per frame over its used points, in float64:
 *     t1, t2 = means;  a = gt - t1, b = pred - t2;  s1 = |a|_F + 1e-8, s2 = |b|_F + 1e-8;  M = (a / s1)^T (b / s2) = U W V^T;
 *     R = U V^T (NO determinant correction: a mirrored prediction is aligned by a reflection, as scipy does), s = sum W;
 *     aligned = ((b / s2) R^T) s s1 + t1.
 *   The SVD is a one-sided Jacobi iteration; a vanishing singular value (three points, coplanar sets) gets its left vector completed
 *   so that U stays orthogonal (its sign does not reach `aligned`: b has no component along it).
 *   aligned NULL or (N,K,3) float32; err (N,K) float32 = |gt - aligned| from the float64 values, rounded once; both NaN at points not
 *   used.  trafo NULL or (N,14) float64: R row-major, s, s1, t1 - t2 (the tuple of return_trafo=True).  n_valid (N) int32.
 *   A frame with fewer than 3 used points has NaN aligned / err / trafo and its true count (the "invalid ground truth" of :204-207).
 *   Returns HARP_ERR_ARG without launching for NULL gt / pred / err / n_valid, N, K, Kp <= 0, or Kp != K without pred_idx.
 *
 * harp_pck_counts replaces the counting of EvalUtil._get_pck / _get_epe / get_measures (utils/eval_util.py:103-163): one workgroup per
 * keypoint.  err (N,K) float32, valid NULL or (N,K) float32 (non-zero = visible), thresholds (n_thr) float32 ON THE DEVICE.  A
 * measurement is seen when it is visible and not NaN.  counts (K,n_thr) int32 = seen n with err[n][k] <= thresholds[j] (the float32
 * comparison), n_vis (K) int32 = seen n, err_sum (K) float64 = their sum.
 *   Returns HARP_ERR_ARG without launching for NULL err / thresholds / counts / n_vis / err_sum, N, K <= 0 or n_thr < 1.
 *
 * harp_point_set_fscore: precision / recall / F between two point sets per frame (the mesh measure of the FreiHAND benchmark, whose
 * helpers the reference ships in utils/fh_utils.py; it complements the vertex error of optimize_sequence.py:760-774).  gt (N,Kg,3),
 * pred (N,Kp,3), thresholds (n_thr) float32 on the device.  In float64: d2(p, q) = sum (double(p) - double(q))^2, nn_gt[n][i] = min over
 * the pred points, nn_pred[n][j] = min over the gt points; per threshold t: precision = share of gt points with nn_gt < double(t)^2,
 * recall = share of pred points with nn_pred < double(t)^2 (strict), F = 2 p r / (p + r), 0 when p + r = 0.
 *   out (N,n_thr,3) float32 (precision, recall, F); nn_gt NULL or (N,Kg), nn_pred NULL or (N,Kp) float32 = the square roots.
 *   All pairs, one workgroup per frame, the other set tiled through LDS.
 *   Returns HARP_ERR_ARG without launching for NULL gt / pred / thresholds / out, N, Kg, Kp <= 0, n_thr outside 1..512. */
int harp_procrustes_align(const float* gt, const float* pred, const int32_t* pred_idx, const float* valid, int N, int K, int Kp,
                          float* aligned, float* err, double* trafo, int32_t* n_valid, hipStream_t stream);
int harp_pck_counts(const float* err, const float* valid, const float* thresholds, int N, int K, int n_thr, int32_t* counts, int32_t* n_vis,
                    double* err_sum, hipStream_t stream);
int harp_point_set_fscore(const float* gt, const float* pred, const float* thresholds, int N, int Kg, int Kp, int n_thr, float* out,
                          float* nn_gt, float* nn_pred, hipStream_t stream);

/* ---- what a fitting job is fed with: decoded uint8 frames -> the resident float32 targets (csrc/ingest.hip) -----------------------------
 * harp_targets_from_u8 replaces everything behind the image decoder in utils/data_util.py:11-51 (load_img called three times per frame by
 * ImagesDataset.__getitem__: `/ 255` in float64, `[::d, ::d]`, cv2.erode(mask, ones((3,3)), iterations=2), torch.Tensor) for N frames in
 * one launch.  rgb (N,H0,W0,3) and mask (N,H0,W0) uint8, contiguous; H = ceil(H0 / d), W = ceil(W0 / d); output pixel (y, x) reads source
 * pixel (y d, x d), the subsampling taken BEFORE the erosion as in load_img.
 *   y_true (N,H,W,3), y_sil (N,H,W) float32 = (float)u / 255.0f, the correctly rounded IEEE float32 division — for each of the 256 codes
 *     the bits of float32(float64(u) / 255.0), which is what the reference's numpy division followed by torch.Tensor yields.
 *   y_sil_col NULL (the erosion is skipped) or (N,H,W) float32 = the same conversion of the minimum of the subsampled mask over the 5 x 5
 *     window clipped to the H x W image = two passes of the 3 x 3 erosion with out-of-image neighbours ignored (cv2's default border).
 *   Outputs need only float alignment (a slice [n0 : n0 + N] of a larger buffer is fine); 16-byte aligned rows leave as 128-bit stores.
 *   Stream-ordered and capturable: no allocation, no workspace, no synchronisation.  Deterministic: no atomics.
 *   Returns HARP_ERR_ARG without launching for NULL rgb / mask / y_true / y_sil, N, H0, W0 <= 0, d outside 1..8, or more than 2^31 - 1 tiles of
 *   16 x 64 output pixels over all frames (the grid; it also keeps every element count below 2^49). */
int harp_targets_from_u8(const unsigned char* rgb, const unsigned char* mask, int N, int H0, int W0, int d, float* y_true, float* y_sil,
                         float* y_sil_col, hipStream_t stream);

/* ---- the frames baked into UV space: texel map, per-texel accumulation, finish, seam dilation (csrc/bake.hip) ---------------------------
 * The reference starts every texture from one flat colour (optimize_sequence.py:234), writes the fitted one multiplied by uv_mask
 * (:627-654) and exports it as it is (:776-791, black outside the charts); it has no map from the atlas back to the frames.  These four are
 * that map.  Forward only.  Every call only enqueues on `stream` and is capturable: no allocation, no synchronisation.  No float atomics
 * (the texel map uses an integer atomicMin, whose result does not depend on the order) and a fixed order in every sum: a repeated call
 * gives the same bits.  Every index read from device memory (texel list, face, vertex, target row) is range-checked before it is used;
 * an entry that fails the check contributes nothing.
 *
 * harp_uv_texel_map rasterises the UV triangles at the texel centres of an (Ht, Wt) atlas.  verts_uvs (VT,2) float32, faces_uvs (F,3) int32.
 *   Texel (x, y) <-> u = x / (Wt - 1), v = 1 - y / (Ht - 1): where the shader's bilinear lookup puts an integer sample.  In texel
 *   coordinates (float32) with e0 = (p1 - c) x (p2 - c), e1 = (p2 - c) x (p0 - c), e2 = (p0 - c) x (p1 - c), area = (p1 - p0) x (p2 - p0),
 *   bi = ei / area: the centre c is inside the face when all three bi >= 0.  Several faces: the LOWEST face index owns the texel.
 *   Zero-area (and non-finite) faces own nothing; faces partly outside [0,1]^2 are clipped to the atlas.
 *   texel_face (Ht*Wt) int32: the owning face or -1; texel_bary (Ht*Wt,2) float32: b0, b1 (b2 = 1 - b0 - b1), 0 where no face.
 *   One wave per face over the texels of its bounding box (no texel walks all faces).
 *   Returns HARP_ERR_ARG without launching for NULL pointers, F < 1, VT < 1, Ht < 2, Wt < 2, Ht * Wt > 2^31 - 257.
 *
 * harp_texture_bake_accum adds the B frames of one call to the per-texel accumulators (harp_bake_args below).  For texel t (entry of
 *   texel_idx, or every texel when it is NULL and n = Ht * Wt) with face f = texel_face[t] >= 0, barycentrics b and the face's vertices
 *   i = faces[f], for frame k = 0 .. B - 1 in this order, in float64:
 *     z = sum bi z_i;  x = sum bi x_i z_i / z, y likewise (ndc (B,V,3) = (x_ndc, y_ndc, z_view) of harp_project_fwd);
 *     fx = (1 - x) S / 2, fy = (1 - y) S / 2;  pixel (ix, iy) = floor;  continuous pixel coordinate (fx - 0.5, fy - 0.5).
 *   The texel is OBSERVED in frame k iff rows[k] is in [0, N), z > 0, 0 <= fx, fy < S, face_id[k][iy][ix] >= 0,
 *     z <= zbuf[k][iy][ix] (1 + depth_tol), y_mask[rows[k]][iy][ix] >= 0.5 and, with verts / vnormals / cam_pos given,
 *     cosv = n^ . v^ >= cos_min, n^ = the interpolated vertex normal and v^ = cam_pos[k] - (interpolated position), each divided by
 *     max(length, 1e-6).  Weight w = max(cosv, 0)^cos_power, or 1 without normals (then cosv counts as 1).
 *   Colour: the bilinear sample of y_true[rows[k]] at the continuous pixel coordinate clamped to [0, S - 1]; with light_pos / colors given
 *     channel c becomes (c - colors[k][6 + c]) / max(colors[k][c] + colors[k][3 + c] max(n^ . l^, 0), shade_floor), l^ towards light_pos[k]:
 *     the inverse of the shader's `lightc * texel + specular` (shade.hip) without shadow and normal map; the specular term is the constant
 *     of shininess 0, and 0 in the fit's shadow renderer.
 *   sum_w += w, sum_wc[c] += w v_c, sum_wc2[c] += w v_c^2 (float64), count += 1, best_cos = max(best_cos, cosv).  The texel's one thread
 *   reads its accumulators, adds the frames one by one and writes them back: the result is the same bits however a sequence is cut into
 *   calls.  texel_idx must hold every texel AT MOST ONCE (the list of a `nonzero`): two entries for one texel would be two threads
 *   reading and writing the same accumulators without atomics.  Returns HARP_ERR_ARG without launching for a NULL struct or required pointer, n, F, V, B, S, N < 1, Ht, Wt < 2, a NULL
 *   texel_idx with n != Ht * Wt, verts / vnormals / cam_pos or light_pos / colors given in part, light without normals, depth_tol < 0,
 *   shade_floor <= 0, cos_power < 0, cos_min < -1 (or NaN for any of the four).
 *
 * harp_texture_bake_finish: seen (Ht*Wt) uint8 = count >= min_count && sum_w > 0; mean (Ht*Wt,3) float32 = clamp(sum_wc / sum_w, 0, 1),
 *   var (NULL ok) = max(sum_wc2 / sum_w - (sum_wc / sum_w)^2, 0); 0 for both where not seen.
 *   Returns HARP_ERR_ARG without launching for NULL sums / count / mean / seen, Ht < 1, Wt < 1.
 *
 * harp_texture_dilate: n_pass Jacobi passes over tex (Ht,Wt,C) float32, C = 1..4, and valid (Ht,Wt) uint8.  Per pass an invalid texel with
 *   at least one valid 8-neighbour becomes the mean of its valid neighbours — summed in float32 in row-major window order, divided once
 *   (correctly rounded) — and is valid from the next pass on.  Valid texels never change; out-of-atlas neighbours are ignored.  allow NULL
 *   or (Ht,Wt) uint8: texels with allow == 0 are never filled and never serve as sources.  Texels still invalid at the end keep their
 *   input value.  One launch per pass, ping-pong through ws = harp_texture_dilate_ws_bytes(Ht, Wt, C) bytes (256-B aligned, no initial
 *   contents), then one copy into out (and valid_out, NULL ok: the final validity).  n_pass = 0 copies bit for bit.  out may alias tex,
 *   valid_out may alias valid.  Returns HARP_ERR_ARG without launching for NULL tex / valid / out, Ht, Wt < 1, C outside 1..4,
 *   n_pass < 0, NULL ws with n_pass > 0.
 * harp_texture_dilate_ws_bytes: pure host arithmetic, 2 * (4 C Ht Wt rounded up to 256) + 2 * (Ht Wt rounded up to 256); 0 for sizes the
 *   call refuses. */
typedef struct {
  const int32_t* texel_idx;   /* (n) covered texels, or NULL = all Ht * Wt */
  const int32_t* texel_face;  /* (Ht*Wt) of harp_uv_texel_map */
  const float* texel_bary;    /* (Ht*Wt,2) */
  const int32_t* faces;       /* (F,3) mesh faces (vertex indices into ndc / verts / vnormals) */
  const float* ndc;           /* (B,V,3) */
  const int32_t* face_id;     /* (B,S,S) hard camera pass */
  const float* zbuf;          /* (B,S,S) */
  const float* y_true;        /* (N,S,S,3) */
  const float* y_mask;        /* (N,S,S) */
  const int32_t* rows;        /* (B) rows of y_true / y_mask */
  const float* verts;         /* (B,V,3) world positions, or NULL */
  const float* vnormals;      /* (B,V,3), or NULL */
  const float* cam_pos;       /* (B,3) world camera centres, or NULL */
  const float* light_pos;     /* (B,3), or NULL */
  const float* colors;        /* (B,9) ambient | diffuse | specular, or NULL */
  double* sum_w;              /* (Ht*Wt) (+=) */
  double* sum_wc;             /* (Ht*Wt,3) (+=) */
  double* sum_wc2;            /* (Ht*Wt,3) (+=) */
  int32_t* count;             /* (Ht*Wt) (+=) */
  float* best_cos;            /* (Ht*Wt) running maximum */
  int n, Ht, Wt, F, V, B, S, N;
  float depth_tol, cos_min, cos_power, shade_floor;
} harp_bake_args;
int harp_uv_texel_map(const float* verts_uvs, const int32_t* faces_uvs, int F, int VT, int Ht, int Wt, int32_t* texel_face, float* texel_bary,
                      hipStream_t stream);
int harp_texture_bake_accum(const harp_bake_args* args, hipStream_t stream);
int harp_texture_bake_finish(const double* sum_w, const double* sum_wc, const double* sum_wc2, const int32_t* count, int Ht, int Wt, int min_count,
                             float* mean, float* var, unsigned char* seen, hipStream_t stream);
size_t harp_texture_dilate_ws_bytes(int Ht, int Wt, int C);
int harp_texture_dilate(const float* tex, const unsigned char* valid, const unsigned char* allow, int Ht, int Wt, int C, int n_pass, float* out,
                        unsigned char* valid_out, void* ws, hipStream_t stream);

/* ---- playback of a fitted avatar (csrc/playback.hip; harp_amd/playback.py) ------------------------------------------------
 * The forward-only player stands in for the way the reference animates and shows a fit: utils/visualize.py:111-143 `change_pose`
 * (pose rows overwritten by hand, then prepare_mesh) and the render calls of :258-320 (render_image / render_image_with_RT, followed by
 * `(img * 255).astype(np.uint8)` on the host).  It strings together harp_hand_front_fwd / harp_arm_front_fwd over a harp_frame_tables that
 * holds the MOTION's rows, harp_raster_setup_pair, harp_rasterize_fwd, harp_rasterize_fwd_keep and harp_shade_fwd — all with NULL
 * gradient pointers — and the two entries below.
 *
 * harp_motion_resample: keys (Tk, 3 n_rot + n_lin) = n_rot axis-angle triples, then n_lin linear channels (trans, cam, light) ->
 * out (Tn, 3 n_rot + n_lin) at times (Tn,) in key-frame units.  Per row: t = fminf(fmaxf(time, 0), Tk - 1) (a NaN time is row 0),
 * k = min((int)t, Tk - 2), f = t - k; f == 0 / f == 1 copy row k / k + 1 bit for bit (resampling at the key times is the identity; Tk == 1:
 * every row is row 0).  Otherwise a rotation is rot_offset (3 n_rot, or NULL) + triple -> quaternion (sin(th/2)/th = 0.5 - th^2/48 below
 * th = 1e-4), q1 negated when q0.q1 < 0 (the shortest arc ON ROTATIONS: an axis-angle of 4 rad is the rotation it is), nlerp when
 * q0.q1 > 0.9995 and slerp otherwise, normalised, back with w >= 0 as 2 atan2(|v|, w) v / |v| (2 v when |v| < 1e-8), minus rot_offset;
 * a linear channel is (1 - f) a + f b.  rot_offset: MANO's 15 finger joints are stored relative to hands_mean (csrc/lbs.hip:35), so the
 * stored numbers are not the joint rotations — pass [0,0,0 | hands_mean], or the matching slice of harp_tree_model.pose_mean.
 * Tk <= 0, Tn <= 0, n_rot < 0, n_lin < 0, n_rot + n_lin == 0 or a NULL keys / times / out: HARP_ERR_ARG before any launch. */
int harp_motion_resample(const float* keys, int Tk, int n_rot, int n_lin, const float* rot_offset, const float* times, int Tn, float* out,
                         hipStream_t stream);
/* rgb (B, S ss, S ss, 3) and face_id (B, S ss, S ss) as harp_shade_fwd and the camera-view harp_rasterize_fwd leave them (a sub-pixel is
 * covered when face_id >= 0), ss in 1..4 -> out (B,S,S,channels) uint8, channels 3 or 4.  Background of frame b: row bg_rows[b] of
 * bg (n_bg,S,S,3) uint8; bg_rows == NULL: row b when n_bg == B, row 0 when n_bg == 1 (any other n_bg: HARP_ERR_ARG).  A row outside
 * [0, n_bg), or bg == NULL (n_bg and bg_rows are then ignored), takes bg_color — 3 floats in [0,1] ON THE DEVICE, quantised like a
 * pixel, (int)(255 clamp01(c) + 0.5), and from there on treated as an image's byte.
 * Per pixel with n covered sub-pixels of ss^2: n == 0 copies the background byte; otherwise
 * v_c = (sum over covered of clamp01(rgb_c) + (ss^2 - n) bg_c / 255) / ss^2, out_c = (int)(255 v_c + 0.5) clamped to 0..255, with
 * clamp01(x) = fminf(fmaxf(x, 0), 1) (a NaN colour is 0).  Alpha (channels == 4) = (255 n + ss^2 / 2) / ss^2 in INTEGER arithmetic:
 * 255 n / ss^2 sits exactly on .5 for (ss, n) = (2, 2) and (4, 8).  Argument errors return before a launch. */
int harp_resolve_u8(const float* rgb, const int32_t* face_id, int B, int S, int ss, const unsigned char* bg, int n_bg, const int32_t* bg_rows,
                    const float* bg_color, int channels, unsigned char* out, hipStream_t stream);

/* ---- scene playback: several avatars in one frame with depth-correct occlusion (csrc/composite.hip; playback.py ScenePlayer) ----
 * All players of one video share the camera (img_size, focal_length; the translation comes from cam), so the view depths that the
 * camera-view harp_rasterize_fwd writes into zbuf are comparable sub-sample by sub-sample.  A LEFT hand is a right-hand fit of
 * horizontally mirrored frames (the model is MANO / SMPL-X right), shown with flip_x: its layer, light included, is mirrored back. */
typedef struct harp_layer {
  const float* rgb;    /* (B, S ss, S ss, 3) as harp_shade_fwd leaves it */
  const float* zbuf;   /* (B, S ss, S ss) view depth as the camera-view harp_rasterize_fwd leaves it (-1 = empty) */
  int32_t flip_x;      /* != 0: the layer is read mirrored, sub-column S ss - 1 - X */
  int32_t reserved;    /* 0 */
} harp_layer;
/* layers: a HOST array of n_layers in 1..4 entries, read during the call and passed to the kernel by value (nothing on the device points
 * at host memory; a captured graph keeps working).  ss in 1..4 -> out (B,S,S,channels) uint8, channels 3 or 4, and, when owner != NULL,
 * owner (B,S,S) uint8.  Output pixel (b, y, x), sub-sample (sy, sx) in [0, ss)^2, output-space sub-pixel (Y, X) = (y ss + sy, x ss + sx):
 *   covered: layer l is read at (b, Y, X), or at (b, Y, S ss - 1 - X) when flip_x; z_l = its zbuf there; the layer is a CANDIDATE when
 *     z_l > 0 (a NaN or -1 is not).
 *   scene depth: scene_z (n_scene,S,S) float32 at OUTPUT resolution, in zbuf's unit; frame b uses row scene_rows[b]; scene_rows == NULL:
 *     row b when n_scene == B, row 0 when n_scene == 1 (any other n_scene: HARP_ERR_ARG).  A row outside [0, n_scene), or scene_z ==
 *     NULL (n_scene and scene_rows are then ignored), means no scene depth.  d = the value at (y, x) is valid when d > 0 (a NaN or 0:
 *     no measurement, nothing in front); when d is valid a candidate needs z_l < d.
 *   winner: the candidate with the smallest z_l, among exactly equal depths the lower layer index.  A sub-sample with a winner is
 *     covered and contributes clamp01(rgb_winner), clamp01(x) = fminf(fmaxf(x, 0), 1) (a NaN colour is 0).
 *   colour: as harp_resolve_u8 with n = the covered sub-samples of ss^2: n == 0 copies the background byte; otherwise
 *     v_c = (sum + (ss^2 - n) bg_c / 255) / ss^2, out_c = (int)(255 v_c + 0.5) clamped to 0..255; the sum in float32 in row-major order
 *     of the OUTPUT sub-samples (sy outer, sx inner; the same order for a flipped layer).  bg, n_bg, bg_rows, bg_color: harp_resolve_u8's
 *     rules; backgrounds are never flipped.  Alpha (channels == 4) = (255 n + ss^2 / 2) / ss^2 in integers.
 *   owner: 0 when n == 0, otherwise 1 + the index of the layer that won the most sub-samples of the pixel (a tie: the lower index) —
 *     the per-hand segmentation of the finished frame.
 * With one unflipped layer, no scene depth and zbuf > 0 <=> face_id >= 0 the bytes are harp_resolve_u8's; a flipped layer gives the
 * bytes of the same call on arrays mirrored beforehand.
 * HARP_ERR_ARG before any launch: layers, out or bg_color NULL; n_layers outside 1..4; a layer with a NULL rgb or zbuf or a non-zero
 * reserved; B, S <= 0, ss outside 1..4, channels not 3 or 4, S ss > 46340, n_bg / n_scene as above. */
int harp_composite_layers_u8(const harp_layer* layers, int n_layers, int B, int S, int ss, const float* scene_z, int n_scene,
                             const int32_t* scene_rows, const unsigned char* bg, int n_bg, const int32_t* bg_rows, const float* bg_color,
                             int channels, unsigned char* out, unsigned char* owner, hipStream_t stream);

/* ---- labelled playback: what the frames show (csrc/annotate.hip; playback/player.py annotate) ----
 * Nothing in the reference does this.  Both entries read what a player's batch leaves on the device, allocate nothing, only enqueue on
 * `stream` and are capturable; the layer array is a HOST array read during the call and passed to the kernel by value, as harp_layer. */
typedef struct harp_label_layer {
  const int32_t* face_id;          /* (B, S ss, S ss) as the camera-view harp_rasterize_fwd leaves it */
  const float* zbuf;               /* (B, S ss, S ss) view depth, as harp_layer's */
  const unsigned char* face_label; /* (F,) the part of every face, 1..255 (playback/labels.py face_part_labels) */
  const float* ndc;                /* (B,V,3) as harp_project_fwd leaves it        \                                       */
  const int32_t* faces;            /* (F,3)                                         | read for the uv output only: all four */
  const float* verts_uvs;          /* (Vt,2)                                        | may be NULL without it                */
  const int32_t* faces_uvs;        /* (F,3)                                        /                                       */
  int32_t V, F, Vt;                /* F > 0 always; V, Vt > 0 with the uv output */
  int32_t flip_x;                  /* != 0: the layer is read mirrored, sub-column S ss - 1 - X */
  int32_t reserved;                /* 0 */
} harp_label_layer;
/* harp_annotate_layers: n_layers in 1..4, ss in 1..4, scene_z / n_scene / scene_rows exactly as harp_composite_layers_u8 -> any of
 * owner (B,S,S) u8, part (B,S,S) u8, depth (B,S,S) f32, face (B,S,S) i32, uv (B,S,S,2) f32, bbox (B,n_layers,4) i32 (each may be NULL, not
 * all).  Output pixel (b, y, x), sub-sample (sy, sx) in [0, ss)^2:
 *   winner per sub-sample: harp_composite_layers_u8's rule, word for word (candidate when z_l > 0, in front of a valid scene depth, the
 *     smallest z, ties to the lower layer; a flipped layer is read at column S ss - 1 - X).  The winner's LABEL is face_label[face_id] of
 *     that layer there, and 0 for a face_id outside [0, F) (nothing is read out of bounds).
 *   owner: 0 when no sub-sample has a winner, otherwise 1 + the layer that won the most sub-samples, a tie to the lower index: bit for
 *     bit harp_composite_layers_u8's owner for the same inputs.
 *   part: among the sub-samples the owner layer won the most frequent label, a tie to the lower label; 0 when owner is 0.
 *   representative sub-sample: among the owner's sub-samples with that label the one with the smallest z, a tie to the first in row-major
 *     order (sy outer, sx inner).  depth = its z (0 when owner is 0); face = its face_id (-1 when owner is 0);
 *     uv = sum_k b_k verts_uvs[faces_uvs[face, k]], and (0, 0) when owner is 0, when face is outside [0, F) or when one of the face's six
 *     table entries is outside [0, V) / [0, Vt).  b = the perspective-corrected barycentrics of csrc/shade_common.h bary_fwd (the same
 *     formula, kEps included) on the face's three ndc rows, at the centre of the SOURCE sub-pixel the layer was read at — the mirrored
 *     column for a flipped layer, the UV belongs to the surface point — in the rasteriser's convention, 1 - 2 (i + 0.5) / (S ss).
 *   bbox (+= by integer atomic max; the caller zeroes it): (S - xmin, S - ymin, xmax + 1, ymax + 1) over the pixels whose owner is
 *     1 + l; all zeros: layer l owns no pixel.
 * HARP_ERR_ARG before any launch: layers NULL; every output NULL; n_layers outside 1..4; a layer with a NULL face_id, zbuf or face_label,
 * F <= 0 or a non-zero reserved; with uv, a layer with a NULL ndc, faces, verts_uvs or faces_uvs or V, Vt <= 0; B, S <= 0; ss outside
 * 1..4; S ss > 46340; n_scene as harp_composite_layers_u8. */
int harp_annotate_layers(const harp_label_layer* layers, int n_layers, int B, int S, int ss, const float* scene_z, int n_scene,
                         const int32_t* scene_rows, unsigned char* owner, unsigned char* part, float* depth, int32_t* face, float* uv,
                         int32_t* bbox, hipStream_t stream);
/* harp_keypoint_visibility: the joints of layer `self_layer` projected and tested against the scene.  joints (B,NJ,3) metres, as the fused
 * front leaves joints_m; cam_R (B,9), cam_T (B,3); focal and S of the OUTPUT image; of the layers only zbuf (B, S ss, S ss) and flip_x are
 * read; tol metres -> uvz (B,NJ,3) f32 and vis (B,NJ,2) u8.  Per joint, with view = harp_project_fwd's transform of j (for its R =
 * diag(-1,-1,1) and T = (-cam1, -cam2, t_z) this is playback/keypoints.py project_pixels): Z = view.z, u = S/2 - focal view.x / Z,
 * v = S/2 - focal view.y / Z, and u becomes S - u when self_layer is flipped.  uvz = (u, v, Z), or zeros when not Z > 1e-3 (a NaN too).
 *   vis[0]: 0 = not in the image (not Z > 1e-3, Z infinite, u or v outside [0, S) or NaN); 1 = hidden; 2 = visible.
 *   vis[1]: what hides it: 0 nothing, 1 + the layer, 255 the scene depth.
 * The test is made at sub-pixel (Y, X) = (min((int)(v ss), S ss - 1), min((int)(u ss), S ss - 1)) of the output frame: the nearest surface
 * there is harp_composite_layers_u8's winner when there is one, otherwise the scene depth at (Y / ss, X / ss) when valid, otherwise
 * nothing.  The joint is visible when there is nothing or z_near >= Z - tol; a joint behind its own skin by more than tol reports its
 * own layer.  HARP_ERR_ARG before any launch: a NULL joints, cam_R, cam_T, layers, uvz or vis; n_layers outside 1..4; self_layer outside
 * [0, n_layers); a layer with a NULL zbuf or a non-zero reserved; B, NJ, S <= 0; ss outside 1..4; S ss > 46340; focal not > 0; tol not
 * >= 0; n_scene as harp_composite_layers_u8. */
int harp_keypoint_visibility(const float* joints, const float* cam_R, const float* cam_T, int B, int NJ, float focal, int S, int ss,
                             int self_layer, const harp_label_layer* layers, int n_layers, const float* scene_z, int n_scene,
                             const int32_t* scene_rows, float tol, float* uvz, unsigned char* vis, hipStream_t stream);

/* ---- motion labels: per-pixel optical flow and occlusion between frames (csrc/flow.hip; playback/player.py flow) ----
 * Nothing in the reference does this.  The entry reads what a player's batch leaves on the device for the SOURCE frames and copies of ndc
 * and zbuf of the TARGET frames (the same meshes in the other pose / camera); it allocates nothing, only enqueues on `stream`, is
 * capturable and uses no atomics: a repeated call gives the same bits.  The layer array is a HOST array read during the call and passed
 * to the kernel by value, as harp_label_layer. */
typedef struct harp_flow_layer {
  const int32_t* face_id;          /* SOURCE frames (B, S ss, S ss), as harp_label_layer's */
  const float* zbuf;               /* SOURCE (B, S ss, S ss) */
  const unsigned char* face_label; /* (F,) */
  const float* ndc;                /* SOURCE (B,V,3) (x_ndc, y_ndc, z_view) */
  const int32_t* faces;            /* (F,3) */
  const float* ndc_to;             /* TARGET frames (B,V,3): the same mesh, the other pose / camera */
  const float* zbuf_to;            /* TARGET (B, S ss, S ss) view depth of this layer */
  int32_t V, F, flip_x, reserved;  /* reserved 0 */
} harp_flow_layer;
/* harp_flow_layers: n_layers in 1..4, ss in 1..4; scene_z / n_scene / scene_rows (the scene depth of the source frames) and scene_z_to /
 * n_scene_to / scene_rows_to (of the target frames) each exactly as harp_composite_layers_u8; tol metres -> flow (B,S,S,2) f32 output
 * pixels, dz (B,S,S) f32 metres, status (B,S,S,2) u8.  Output pixel (b, y, x):
 *   source point: harp_annotate_layers' winner rule, owner, part and representative sub-sample, word for word, on the source layers and
 *     the source scene depth.  Layer l = owner - 1; face f and depth z are the representative sub-sample's, at output sub-pixel (Y, X);
 *     Xs = the source column the layer was read at (S ss - 1 - X for a flipped layer); b_k = csrc/shade_common.h bary_fwd (kEps included)
 *     on the face's three source ndc rows at the centre of (Y, Xs), 1 - 2 (i + 0.5) / (S ss): exactly the point `uv` is taken at.
 *   target point, (x'_k, y'_k, z'_k) = the face's rows of ndc_to (harp_texture_bake_accum's projection of a barycentric point):
 *     Z' = sum_k b_k z'_k, x' = sum_k b_k x'_k z'_k / Z', y' likewise; cx = (1 - x') S ss / 2, cy = (1 - y') S ss / 2: continuous sub-pixel
 *     coordinates, the centre of sub-pixel i at i + 0.5; for a flipped layer cx := S ss - cx.
 *   flow = ((cx - (X + 0.5)) / ss, (cy - (Y + 0.5)) / ss), dz = Z' - z.
 *   status[0]: 0 = no owner (flow, dz zero); 1 = not trackable: f outside [0, F), a vertex index of the face outside [0, V), not
 *     Z' > 1e-3, or Z', cx or cy not finite (nothing is read out of bounds; flow, dz zero); 2 = lands outside the image, cx or cy outside
 *     [0, S ss) (flow and dz are written); 3 = hidden at the target; 4 = visible at the target.
 *   3 / 4 is harp_keypoint_visibility's test at target sub-pixel (Yt, Xt) = (min((int)cy, S ss - 1), min((int)cx, S ss - 1)): the nearest
 *     surface is the composite's winner over the layers' zbuf_to (a flipped layer read at column S ss - 1 - Xt) in front of the target
 *     scene depth at (Yt / ss, Xt / ss) when there is one, otherwise that scene depth when valid, otherwise nothing; visible when there
 *     is nothing or z_near >= Z' - tol.
 *   status[1]: what hides the point: 0 nothing, 1 + the layer (the point's own layer for self-occlusion), 255 the scene depth.
 * HARP_ERR_ARG before any launch: a NULL layers, flow, dz or status; n_layers outside 1..4; a layer with any NULL pointer, V <= 0, F <= 0
 * or a non-zero reserved; B, S <= 0; ss outside 1..4; S ss > 46340; tol not >= 0 or not finite; n_scene or n_scene_to as
 * harp_composite_layers_u8. */
int harp_flow_layers(const harp_flow_layer* layers, int n_layers, int B, int S, int ss, const float* scene_z, int n_scene,
                     const int32_t* scene_rows, const float* scene_z_to, int n_scene_to, const int32_t* scene_rows_to, float tol, float* flow,
                     float* dz, unsigned char* status, hipStream_t stream);

/* ---- contact labels: per-vertex distance and penetration between two meshes (csrc/contact.hip; playback/player.py ScenePlayer.contact;
 * DESIGN.md §36) ----
 * Nothing in the reference does this.  The entry is pairwise: for every vertex of a QUERY mesh its relation to the surface of a TARGET
 * mesh, over the B frames of a batch.  It uses no atomics, allocates nothing, only enqueues on `stream` (a set-up launch and the main
 * launch) and is capturable; a repeated call gives the same bits.  Both structs are HOST structs read during the call. */
typedef struct harp_contact_mesh {
  const float* verts;     /* (B,V,3) model-space vertices as the fused front leaves `vd` */
  const float* cam_R;     /* (B,9)  \ view = harp_project_fwd's transform: X = p.r[0,3,6] + T[0], Y = p.r[1,4,7] + T[1],    */
  const float* cam_T;     /* (B,3)  / Z = p.r[2,5,8] + T[2]                                                                  */
  const int32_t* faces;   /* (F,3); read for the target only, may be NULL for the query (whose F is not read either) */
  int32_t V, F;
  int32_t flip_x;         /* != 0: the mesh is shown mirrored, view.x -> -view.x */
  int32_t reserved;       /* 0 */
} harp_contact_mesh;
/* floats of workspace for B frames of a target of F_target faces (0 for B <= 0 or F_target <= 0): per frame one box of 8 floats per
 * chunk of 128 faces and 12 floats per face (its view-space corners), written by the set-up launch and read by the main one */
size_t harp_mesh_contact_ws_floats(int B, int F_target);
/* harp_mesh_contact: max_dist metres, ws of harp_mesh_contact_ws_floats(B, target->F) floats, 16-byte aligned -> dist (B,Vq) f32,
 * face (B,Vq) i32, wind (B,Vq) f32.  All geometry is in view space after the flip.  For query vertex (b, i) with view position p:
 *   dist: the unsigned Euclidean distance from p to the nearest point of the target's triangles of frame b when that distance is
 *     <= max_dist, otherwise +inf.  max_dist = +inf is allowed: no limit.
 *   face: a target face that attains that distance, the lowest index among exactly equal float32 values; -1 when dist is +inf.
 *   wind: the generalised winding number of the target surface about p = the sum over the target's faces of the signed solid angle
 *     over 4 pi, in van Oosterom-Strackee form: 2 atan2(det[a,b,c], |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) with a, b, c the corners
 *     minus p.  It is negated when target->flip_x is set (mirroring reverses the orientation).  It is computed only where dist is
 *     finite and is 0 elsewhere.  About 1 inside a closed outward-oriented mesh and about 0 outside; MANO and the arm mesh are open at
 *     the wrist or shoulder, so the value is fractional near the opening.  "Inside" as wind > 0.5 is the Python layer's convention.
 *   A target face with a non-finite corner (in view space) or an index outside [0, target->V) is skipped by both sums; nothing is read
 *     out of bounds.  A zero-area face (its normal (b - a) x (c - a) exactly zero in float32, as for repeated indices) counts as its
 *     segment or point for the distance and adds 0 to wind; no input gives a NaN.  A non-finite query vertex gives +inf, -1, 0.
 *   dist, face and wind may each be NULL, but not all three; a missing output changes nothing in the others.
 * The distance is computed in float32 from the float32 view positions: within 32 * 2^-24 M of the exact one, M the largest absolute view
 * coordinate.  The result does not depend on how the faces are chunked: chunks are skipped by bounding boxes only where no face of
 * theirs could replace or tie a result.
 * HARP_ERR_ARG before any launch: a NULL query, target, ws, verts, cam_R or cam_T; a NULL target->faces; V of either, target->F or B <= 0;
 * a non-zero reserved; max_dist negative or NaN; all outputs NULL; ws not 16-byte aligned; more than 2^31 - 1 tiles of 64 query vertices
 * or chunks over the batch. */
int harp_mesh_contact(const harp_contact_mesh* query, const harp_contact_mesh* target, int B, float max_dist, float* ws, float* dist,
                      int32_t* face, float* wind, hipStream_t stream);

/* ---- the same with a per-(query vertex, target face) exclusion: self-contact within one mesh (csrc/contact.hip; playback/player.py
 * self_contact) ----
 * A vertex of a mesh is at distance 0 from its own faces, so a mesh queried against itself needs to be told which faces do not count
 * for which vertex (playback/selfcontact.py builds the table from a geodesic radius).
 * Table: excl[(c * V_query + i) * 4 + (k >> 5)] bit (k & 31) stands for target face c * HARP_CONTACT_EXCL_FACES + k and query vertex i:
 * chunk-major, one 16-byte word of 128 bits per (chunk of 128 faces, vertex), so that the 64 lanes of a tile read 64 consecutive words
 * per chunk.  harp_contact_excl_words(V_query, F_target) = ceil(F_target / 128) * V_query * 4 uint32 words (0 for a non-positive
 * argument).  The table is the same for every frame of the batch: it belongs to a topology, not to a pose.  Bits past F are ignored. */
#define HARP_CONTACT_EXCL_FACES 128
size_t harp_contact_excl_words(int V_query, int F_target);
/* harp_mesh_contact_excl: harp_mesh_contact's contract word for word (the same ws of harp_mesh_contact_ws_floats floats, the same two
 * launches, no atomics, no allocation, capturable, a repeated call gives the same bits), with one addition: a face whose bit is set for
 * a query vertex is skipped by that vertex's distance MINIMUM.  That decides dist, face (the lowest index among the faces that count
 * and attain the minimum), and whether the vertex is within max_dist; a vertex with every valid face excluded gives +inf, -1, 0.
 *   wind is NOT masked: it is the sum over ALL valid faces of the target, computed only where the masked dist is within max_dist.  For
 *     a vertex ON the surface of its own closed mesh that sum is the vertex's exterior-angle share (the faces that meet at it add
 *     exactly 0, the rest of the surface is seen under less than a half space from a convex place, more from a concave one): 0.14 .. 0.82
 *     on the hand template at rest, no vertex above 0.95, and it rises by about 1 when the vertex is inside ANOTHER part of the mesh
 *     (two overlapping 320-face icospheres as one mesh: 0.415 .. 0.421 outside, 1.415 .. 1.421 inside) — so "inside" is wind > 1.0 here,
 *     the Python layer's convention.  A MASKED winding sum has no such reading: from a convex patch its own neighbourhood is seen
 *     edge-on, so what removing it takes from the sum depends on the radius of the exclusion.
 * HARP_ERR_ARG before any launch: harp_mesh_contact's, and a NULL excl or one that is not 16-byte aligned. */
int harp_mesh_contact_excl(const harp_contact_mesh* query, const harp_contact_mesh* target, const uint32_t* excl, int B, float max_dist,
                           float* ws, float* dist, int32_t* face, float* wind, hipStream_t stream);

/* ---- batched MANO inverse kinematics: 3-D keypoints -> pose rows (csrc/ik.hip; playback.py Motion.from_keypoints) ----
 * Nothing in the reference does this: its change_pose takes another sequence's parameters.  The model inverted is harp_lbs_mano_fwd's.
 * T independent Levenberg-Marquardt solves in one launch, forward only, no workspace, no allocation, no synchronisation, no atomics
 * (capturable; a repeated call gives the same bits).  Unknowns per frame x = [rot 3 | pose 45 | trans 3] = the rows of pose48 and trans
 * as harp_lbs_mano_fwd takes them; the shape is given: betas (10,) for all frames, or (T,10) with betas_per_frame != 0.
 *   j(x) (21,3) metres = harp_lbs_mano_fwd's joints / 1000.
 *   C(x) = sum_k w_k |j_k(x) - t_k|^2 + prior_weight sum_i (pose_i - prior_i)^2; targets (T,21,3) metres; weights (T,21) or NULL (ones);
 *   prior (T,45) or NULL (zeros: the model's mean pose).  A joint is USED when w_k > 0 and its three target coordinates are finite; an
 *   unused joint's target never enters arithmetic.
 *   Iteration, exactly `iters` times: J = the exact 63 x 51 derivative of j at x; A = J^T W J + P, g = J^T W r + P (x - prior), P =
 *   prior_weight on the 45 pose diagonals; (A + lambda diag A) d = -g by a Cholesky factorisation of the matrix scaled from both sides by
 *   1 / sqrt(A_ii (1 + lambda)); x' = x + d; C(x') < C(x): accept, lambda = max(0.1 lambda, 1e-9); otherwise (a NaN included, and a
 *   non-positive or non-finite pivot or diagonal) keep x, lambda = min(10 lambda, 1e6).  lambda starts at lambda0.
 * In/out: pose48 (T,48), trans (T,3).  Out: cost (T,2) = C at the input and at the result; status (T) int32 = accepted steps, or -1 for a
 * frame with fewer than 3 used joints, which is not solved (its pose48 / trans rows are not written).  Optional out (NULL allowed):
 * joints (T,21,3) mm and jac (T,63,51) (metres per unit of x) at the final x.  iters == 0 evaluates cost, joints and jac at the input and
 * writes neither pose48 nor trans.
 * HARP_ERR_ARG before any launch: m, opt, betas, targets, pose48, trans, cost or status NULL; T <= 0; iters < 0; lambda0 or prior_weight
 * negative or not finite.  harp_mano_ik_frames_per_block: the frames one workgroup solves (tests size their batches around it). */
typedef struct harp_ik_options {
  int iters;
  float lambda0;       /* 1e-3 */
  float prior_weight;
  int betas_per_frame; /* 0: betas (10,); otherwise betas (T,10) */
} harp_ik_options;
int harp_mano_ik_frames_per_block(void);
int harp_mano_ik(const harp_mano_model* m, const float* betas, const float* targets, const float* weights, const float* prior, int T,
                 const harp_ik_options* opt, float* pose48, float* trans, float* cost, int32_t* status, float* joints, float* jac,
                 hipStream_t stream);

/* ---- motion smoothing: a confidence-weighted, rotation-aware window filter (csrc/filter.hip; playback.py Motion.smooth, smooth_keypoints;
 * DESIGN.md §25) ----
 * Nothing in the reference does this on the device (its preprocessing removes one-frame jumps of `pose` on the host and otherwise runs an
 * Adam loop over the sequence).  rows (T, W): per row n_rot axis-angle triples | n_vec 3-vectors | n_lin scalars; nch = n_rot + n_vec +
 * n_lin channels, W = 3 (n_rot + n_vec) + n_lin columns.  Out: out (T, W) and used (T, nch) int32.  Forward only; one launch, no
 * workspace, no allocation, no synchronisation, no atomics, no data-dependent exit: two calls give the same bits and the launch can be
 * captured (one kernel node).  Per output row t and channel j:
 *   window: R_t = the largest d <= R such that every row t - d' and t + d', d' <= d, lies in [0, T) and has segment == segment[t]
 *     (segment (T) int32 or NULL: one segment).  The window shrinks on BOTH sides, so a track that is linear in time is reproduced and the
 *     ends of a clip are not pulled along its slope.  Samples are visited in a fixed order — the centre, then d = 1 .. R_t with t - d before
 *     t + d — and every sum below runs in that order, in float32.
 *   sample weights: a_s = taps[|s - t|] c_s in float32, taps (R + 1) by distance; c_s = 1 when weights == NULL (w_cols 0), weights[s]
 *     (w_cols 1) or weights[s nch + j] (w_cols nch).  A tap, a weight or their product that is negative or not finite counts as 0.  A
 *     sample with a_s == 0 or a non-finite value in the channel's columns is UNUSED and never enters arithmetic.
 *   copies: no used sample: the input is copied bit for bit, used = 0.  The centre the only used sample: the input is copied bit for bit,
 *     used = 1 (R == 0 is the identity).
 *   scalar and vector channels: m = sum a_s v_s / sum a_s.  With trim != NULL and trim[j] > 0 the samples with |v_s - m| > trim[j]
 *     (Euclidean for a 3-vector) are left out and, when some but not all remain, m is that mean over the rest.
 *   rotation channels: q_s = quat(triple_s + offset), offset = rot_offset[3 j ..] (rot_offset (3 n_rot) or NULL: zero — MANO's finger rows
 *     are stored relative to hands_mean, harp_motion_resample's rot_offset), with sin(th/2)/th = 0.5 - th^2/48 below th = 1e-4.  Every q_s
 *     whose dot with the FIRST used sample's quaternion is negative is negated.  S = sum a_s q_s; |S| < 1e-6 sum a_s (antipodal samples):
 *     the input is copied, used = -1.  mu = S / |S|; then exactly `iters` times v = sum a_s log(mu^-1 q_s) / sum a_s, mu <- mu exp(v), with
 *     log(q) taken with w >= 0 as 2 atan2(|v|, w) v / |v| (2 v when |v| < 1e-8) and exp = quat.  With trim[j] > 0 the samples farther than
 *     trim[j] radians from mu (|log(mu^-1 q_s)|) are left out and, when some but not all remain, the estimate is computed again from scratch
 *     over them (a vanishing chordal sum there copies the input with used = -1 as well).  out = log(mu) - offset.
 *   trimming that would leave no sample leaves the first estimate; used = the number of samples in the final mean.
 * HARP_ERR_ARG before any launch: rows, taps, out or used NULL; T <= 0; a negative n_rot, n_vec or n_lin; nch == 0; R outside
 * 0..HARP_FILTER_MAX_RADIUS; iters outside 0..8; weights == NULL with w_cols != 0, or weights != NULL with w_cols not 1 or nch; T W beyond
 * the range of an int.  Every gather is row t - d or t + d after 0 <= t - d and t + d < T. */
#define HARP_FILTER_MAX_RADIUS 64
int harp_motion_filter(const float* rows, int T, int n_rot, int n_vec, int n_lin, const float* rot_offset, const float* taps, int R,
                       const float* weights, int w_cols, const int32_t* segment, const float* trim, int iters, float* out, int32_t* used,
                       hipStream_t stream);

/* ---- batched MANO vertex fit: 778 mesh vertices -> pose, shape and trans rows (csrc/vertex_fit.hip; metro_modifications/hand_utils.py
 * optimize_for_mano_param(method="lm"); playback Motion.from_vertices) ----
 * The reference fits these rows with 500 + 700 Adam iterations (metro_modifications/hand_utils.py:16-131).  The model inverted is
 * harp_lbs_mano_fwd's.  T independent Levenberg-Marquardt solves in one launch, forward only, no workspace, no allocation, no
 * synchronisation, no atomics, fixed summation order (capturable; a repeated call gives the same bits).  Unknowns per frame
 * x = [rot 3 | pose 45 | betas 10 | trans 3] = the rows of pose48, betas and trans as harp_lbs_mano_fwd takes them.
 *   solve_shape == 0: betas are given and are not written: (10,) for all frames, or (T,10) with betas_per_frame != 0; their ten columns are
 *   FROZEN.  solve_shape != 0: betas (T,10) are in/out (betas_per_frame is not read).
 *   v(x) (778,3) metres = harp_lbs_mano_fwd's verts / 1000.
 *   C(x) = sum_v w_v |v(x) - t_v|^2 + pose_prior_weight sum_i (pose_i - prior_i)^2 + shape_prior_weight sum_k betas_k^2; targets (T,778,3)
 *   metres; weights (T,778) or NULL (ones); prior (T,45) or NULL (zeros: the model's mean pose).  A vertex is USED when w_v > 0 and its
 *   three target coordinates are finite; an unused vertex's target never enters arithmetic.
 *   Iteration, exactly `iters` times: J = the exact 2334 x 61 derivative of v at x; A = J^T W J + P, g = J^T W r + P (x - x_prior), P = the
 *   two prior weights on the 45 pose and 10 shape diagonals (x_prior: prior for the pose, 0 for the shape); a frozen column has A_ii = 1,
 *   zeros elsewhere in its row and column, and g_i = 0, so its step is exactly 0; (A + lambda diag A) d = -g by a Cholesky factorisation
 *   of the matrix scaled from both sides by 1 / sqrt(A_ii (1 + lambda)); x' = x + d; C(x') < C(x): accept, lambda = max(0.1 lambda, 1e-9);
 *   otherwise (a NaN included, and a non-positive or non-finite pivot or diagonal) keep x, lambda = min(10 lambda, 1e6).  lambda starts
 *   at lambda0.
 * In/out: pose48 (T,48), trans (T,3), betas when solve_shape.  Out: cost (T,2) = C at the input and at the result; status (T) int32 =
 * accepted steps, or -1 for a frame with fewer than 21 used vertices (3 x 21 >= 61), which is not solved (its rows are not written).
 * Optional out (NULL allowed), all at the final x: verts (T,778,3) mm; jac (T,2334,61), metres per unit of x, always all 61 columns; A
 * (T,61,61) and g (T,61), unscaled, frozen columns as above.  iters == 0 evaluates all of them at the input and writes none of the in/out
 * rows.
 * HARP_ERR_ARG before any launch: m, opt, targets, pose48, betas, trans, cost or status NULL; T <= 0; iters < 0; lambda0 or a prior weight
 * negative or not finite.  harp_mano_vertex_fit_frames_per_block: the frames one workgroup solves (tests size their batches around it). */
typedef struct harp_vertex_fit_options {
  int iters;
  float lambda0;            /* 1e-3 */
  float pose_prior_weight;  /* 0: the reference's unregularised MSE */
  float shape_prior_weight; /* 0 */
  int solve_shape;          /* 0: betas given and frozen; otherwise betas (T,10) in/out */
  int betas_per_frame;      /* with solve_shape == 0: 0: betas (10,); otherwise betas (T,10) */
} harp_vertex_fit_options;
int harp_mano_vertex_fit_frames_per_block(void);
int harp_mano_vertex_fit(const harp_mano_model* m, const float* targets, const float* weights, const float* prior, int T,
                         const harp_vertex_fit_options* opt, float* pose48, float* betas, float* trans, float* cost, int32_t* status,
                         float* verts, float* jac, float* A, float* g, hipStream_t stream);

/* ---- batched SMPL-X arm vertex fit: arm or hand mesh vertices -> rot, wrist, pose, shape and trans rows (csrc/arm_vertex_fit.hip;
 * metro_modifications/hand_utils.py optimize_for_mano_arm_param(method="lm"); playback Motion.from_arm_vertices) ----
 * The reference fits these rows with 500 + 700 Adam iterations (metro_modifications/hand_utils.py:134-240).  The model inverted is
 * harp_lbs_tree_fwd's.  T independent Levenberg-Marquardt solves in one launch, forward only, no workspace, no allocation, no
 * synchronisation, no atomics, fixed summation order (capturable; a repeated call gives the same bits).  Unknowns per frame
 * x = [rot 3 | wrist 3 | pose 45 | betas 10 | trans 3]: x[0..51) is the frame's row of in_pose (T,17,3) exactly as harp_lbs_tree_fwd takes
 * it (row pose_src names: 0 = global orient, 1 = right wrist, 2..16 = right hand; stored relative to pose_mean), x[51..61) the first ten
 * shape coefficients, x[61..64) transl.
 *   v(x) (NV,3) metres = harp_lbs_tree_fwd's verts / 1000 for the shape [betas | NB - 10 zeros]: the subtraction of the posed
 *   center_joint and the + transl included.
 *   targets (T,n_t,3) metres: row i belongs to model vertex vert_idx[i] (n_t int32, any order, shared by the frames); vert_idx == NULL:
 *   n_t == NV and the map is the identity.  An index outside [0, NV) is clamped into it: the caller checks the range (ops does).
 *   weights (T,n_t) or NULL (ones); prior (T,45) or NULL (zeros: the model's mean pose).  A target is USED when its weight is > 0 and its
 *   three coordinates are finite; an unused target never enters arithmetic.
 *   C(x) = sum_i w_i |v_{vert_idx[i]}(x) - t_i|^2 + pose_prior_weight sum (pose - prior)^2 + wrist_prior_weight sum wrist^2 +
 *   shape_prior_weight sum betas^2.
 *   solve_shape == 0: betas are given and are not written: (10,) for all frames, or (T,10) with betas_per_frame != 0; their ten columns are
 *   FROZEN.  solve_shape != 0: betas (T,10) are in/out (betas_per_frame is not read).  solve_wrist == 0: the wrist row of in_pose is read
 *   and never written; its three columns are FROZEN.
 *   Iteration, exactly `iters` times, harp_mano_vertex_fit's word for word: J = the exact 3 n_t x 64 derivative of the indexed vertices at
 *   x; A = J^T W J + P, g = J^T W r + P (x - x_prior), P = the three prior weights on the 45 pose, 3 wrist and 10 shape diagonals (x_prior:
 *   prior for the pose, 0 otherwise); a frozen column has A_ii = 1, zeros elsewhere in its row and column, and g_i = 0, so its step is
 *   exactly 0; (A + lambda diag A) d = -g by a Cholesky factorisation of the matrix scaled from both sides by 1 / sqrt(A_ii (1 + lambda));
 *   x' = x + d; C(x') < C(x): accept, lambda = max(0.1 lambda, 1e-9); otherwise (a NaN included, and a non-positive or non-finite pivot or
 *   diagonal) keep x, lambda = min(10 lambda, 1e6).  lambda starts at lambda0.
 * In/out: in_pose (T,17,3) (the wrist row only when solve_wrist), trans (T,3), betas when solve_shape.  Out: cost (T,2) = C at the input
 * and at the result; status (T) int32 = accepted steps; -1 for a frame with fewer than 22 used targets (3 x 22 >= 64), which is not solved
 * (its rows are not written); -2 (cost 0, nothing else written) when the model's tree is not one the kernel's tables hold: row 0 must
 * drive joint 0, every other row a joint of its own below it, and the joints at or below the driven non-root joints, counted per driven
 * joint, must number at most 48 (the arm: 16 for the wrist + 5 x 6 for the fingers).  The skin weights of a vertex must sum to one.
 * Optional out (NULL allowed), all at the final x: verts (T,NV,3) mm, ALL model vertices; jac (T,3 n_t,64), metres per unit of x, always
 * all 64 columns; A (T,64,64) and g (T,64), unscaled, frozen columns as above.  iters == 0 evaluates all of them at the input and writes
 * none of the in/out rows.
 * HARP_ERR_ARG before any launch: m, opt, targets, in_pose, betas, trans, cost or status NULL; T <= 0; iters < 0; n_t < 1 or n_t > NV;
 * vert_idx == NULL with n_t != NV; n_pose_in != 17; NB < 10, NB > 32 or NJ > 64; NV > HARP_ARM_VERTEX_FIT_MAX_VERTS (the per-vertex tables
 * of one frame live in LDS); center_joint outside [0, NJ); lambda0 or a prior weight negative or not finite.
 * harp_arm_vertex_fit_frames_per_block: the frames one workgroup solves (tests size their batches around it). */
#define HARP_ARM_VERTEX_FIT_MAX_VERTS 1088
typedef struct harp_arm_vertex_fit_options {
  int iters;
  float lambda0;            /* 1e-3 */
  float pose_prior_weight;  /* 0: the reference's unregularised MSE */
  float wrist_prior_weight; /* 0 */
  float shape_prior_weight; /* 0 */
  int solve_shape;          /* 0: betas given and frozen; otherwise betas (T,10) in/out */
  int solve_wrist;          /* 0: the wrist row of in_pose given and frozen */
  int betas_per_frame;      /* with solve_shape == 0: 0: betas (10,); otherwise betas (T,10) */
} harp_arm_vertex_fit_options;
int harp_arm_vertex_fit_frames_per_block(void);
int harp_arm_vertex_fit(const harp_tree_model* m, const int32_t* vert_idx, int n_t, const float* targets, const float* weights,
                        const float* prior, int T, const harp_arm_vertex_fit_options* opt, float* in_pose, float* betas, float* trans,
                        float* cost, int32_t* status, float* verts, float* jac, float* A, float* g, hipStream_t stream);

/* ---- batched SMPL-X arm inverse kinematics: 3-D keypoints -> rot, wrist, pose and trans rows (csrc/arm_ik.hip; playback
 * Motion.from_arm_keypoints) ----
 * Nothing in the reference does this.  The model inverted is harp_lbs_tree_fwd's.  T independent Levenberg-Marquardt solves in one launch,
 * forward only, no workspace, no allocation, no synchronisation, no atomics, fixed summation order (capturable; a repeated call gives the
 * same bits).  Unknowns per frame x = [rot 3 | wrist 3 | pose 45 | trans 3]: x[0..51) is the frame's row of in_pose (T,17,3) exactly as
 * harp_lbs_tree_fwd takes it (row pose_src names: 0 = global orient, 1 = right wrist, 2..16 = right hand; stored relative to pose_mean),
 * x[51..54) transl.  The shape is given: betas (10,) for all frames, or (T,10) with betas_per_frame != 0; the model's other NB - 10
 * coefficients are zero.
 *   j(x) (n_out,3) metres = harp_lbs_tree_fwd's joints / 1000, n_out = n_joints_out (the arm: 22 — the wrist, the five fingers root to tip,
 *   the elbow): the subtraction of the posed center_joint and the + transl included.  Row k is joint_src[k]: >= 0 a joint of the tree, < 0 a
 *   skinned vertex (shape blend, the pose correctives of all NJ - 1 joints, skinning over all NJ joints).
 *   C(x) = sum_k w_k |j_k(x) - t_k|^2 + pose_prior_weight sum (pose - prior)^2 + wrist_prior_weight sum (wrist - wrist_prior)^2; targets
 *   (T,n_out,3) metres; weights (T,n_out) or NULL (ones); prior (T,45) or NULL (zeros: the model's mean pose); wrist_prior (T,3) or NULL
 *   (zeros).  A joint is USED when w_k > 0 and its three target coordinates are finite; an unused joint's target never enters arithmetic.
 *   solve_wrist == 0: the wrist row of in_pose is read and never written; its three columns are FROZEN.
 *   Iteration, exactly `iters` times, harp_mano_ik's and harp_arm_vertex_fit's: J = the exact 3 n_out x 54 derivative of j at x; A = J^T W J
 *   + P, g = J^T W r + P (x - x_prior), P = the two prior weights on the 45 pose and 3 wrist diagonals; a frozen column has A_ii = 1, zeros
 *   elsewhere in its row and column, and g_i = 0, so its step is exactly 0; (A + lambda diag A) d = -g by a Cholesky factorisation of the
 *   matrix scaled from both sides by 1 / sqrt(A_ii (1 + lambda)); x' = x + d; C(x') < C(x): accept, lambda = max(0.1 lambda, 1e-9);
 *   otherwise (a NaN included, and a non-positive or non-finite pivot or diagonal) keep x, lambda = min(10 lambda, 1e6).  lambda starts at
 *   lambda0.
 * In/out: in_pose (T,17,3) (the wrist row only when solve_wrist), trans (T,3).  Out: cost (T,2) = C at the input and at the result; status
 * (T) int32 = accepted steps; -1 for a frame with fewer than 3 used joints, which is not solved (its rows are not written); -2 (cost 0,
 * nothing else written) when the model's tree is not one the kernel's tables hold, by harp_arm_vertex_fit's rule: row 0 must drive joint
 * 0, every other row a joint of its own below it, and the joints at or below the driven non-root joints, counted per driven joint, must
 * number at most 48.  The skin weights of a vertex row must sum to one.  Optional out (NULL allowed), at the final x: joints (T,n_out,3)
 * mm and jac (T,3 n_out,54), metres per unit of x, always all 54 columns.  iters == 0 evaluates cost, joints and jac at the input and
 * writes neither in_pose nor trans.
 * HARP_ERR_ARG before any launch: m, opt, betas, targets, in_pose, trans, cost or status NULL; T <= 0; iters < 0; lambda0 or a prior weight
 * negative or not finite; n_joints_out outside 1..HARP_ARM_IK_MAX_JOINTS; center_joint outside [0, NJ); n_pose_in != 17; NB < 10, NB > 32
 * or NJ > 64.  harp_arm_ik_frames_per_block: the frames one workgroup solves (tests size their batches around it). */
#define HARP_ARM_IK_MAX_JOINTS 22
typedef struct harp_arm_ik_options {
  int iters;
  float lambda0;            /* 1e-3 */
  float pose_prior_weight;  /* 0 */
  float wrist_prior_weight; /* 0 */
  int solve_wrist;          /* 0: the wrist row of in_pose given and frozen */
  int betas_per_frame;      /* 0: betas (10,); otherwise betas (T,10) */
} harp_arm_ik_options;
int harp_arm_ik_frames_per_block(void);
int harp_arm_ik(const harp_tree_model* m, const float* betas, const float* targets, const float* weights, const float* prior,
                const float* wrist_prior, int T, const harp_arm_ik_options* opt, float* in_pose, float* trans, float* cost, int32_t* status,
                float* joints, float* jac, hipStream_t stream);

/* ---- batched 2.5-D reprojection IK: image keypoints -> MANO pose rows (csrc/reproj_ik.hip; playback Motion.from_image_keypoints;
 * DESIGN.md §30) ----
 * Nothing in the reference does this.  The model inverted is harp_lbs_mano_fwd's, seen through the player's camera (utils/visualize.py:
 * 268-271: R = diag(-1,-1,1), T = (-cam1, -cam2, t_z)) and the rasteriser's pixel centres.  N independent Levenberg-Marquardt solves in
 * one launch (one kernel node), forward only, no workspace, no allocation, no synchronisation, no atomics, fixed summation order
 * (capturable; a repeated call gives the same bits).  Unknowns per problem x = [rot 3 | pose 45 | trans 3] = the rows of pose48 and trans
 * as harp_lbs_mano_fwd takes them; the shape is given: betas (10,) for all problems, or (N,10) with betas_per_frame != 0; the camera is
 * given: cam (3,), or (N,3) with cam_per_frame != 0, plus focal and S (the image is S x S pixels).
 *   j(x) (21,3) metres = harp_lbs_mano_fwd's joints / 1000 (trans included).
 *   Z_k = j_k.z + t_z, t_z = 2 focal / (S cam0 + 1e-9);   u_k = S/2 + focal (j_k.x + cam1) / Z_k;   v_k = S/2 + focal (j_k.y + cam2) / Z_k;
 *   d_k = j_k.z - j_0.z.   u, v are continuous pixel coordinates: the centre of column i is at u = i + 0.5 and of row i at v = i + 0.5,
 *   u grows with the column and v with the row of the rendered image (harp_project's x_ndc = 1 - 2u/S read at the rasteriser's pixel
 *   centres -1 + (2 (S - 1 - i) + 1) / S).
 *   C(x) = sum_k w_k [(u_k - U_k)^2 + (v_k - V_k)^2] + sum_{k>=1} wz_k (d_k - D_k)^2 + pose_prior_weight sum_i (pose_i - prior_i)^2
 *          + z_prior_weight (trans_z - z_prior)^2;
 *   targets (N,21,3) = (U, V, D): pixels, pixels, metres; weights (N,21) or NULL (ones); depth_weights (N,21) or NULL (no depth rows; the
 *   wrist's own entry is never used); prior (N,45) or NULL (zeros: the model's mean pose); z_prior (N) or NULL (then z_prior_weight must
 *   be 0).  The weights are in px^2 per squared unit of their residual.  A joint's PIXEL rows are used when w_k > 0 and U_k, V_k are finite;
 *   its DEPTH row when k >= 1, wz_k > 0 and D_k is finite; an unused entry never enters arithmetic.
 *   Iteration, exactly `iters` times, harp_mano_ik's: J = the exact 63 x 51 derivative of the rows (u, v, d) at x; A = J^T W J + P,
 *   g = J^T W r + P (x - x_prior), P = pose_prior_weight on the 45 pose diagonals and z_prior_weight on trans_z's; (A + lambda diag A) d =
 *   -g by a Cholesky factorisation of the matrix scaled from both sides by 1 / sqrt(A_ii (1 + lambda)); x' = x + d; C(x') < C(x): accept,
 *   lambda = max(0.1 lambda, 1e-9); otherwise (a NaN included, a non-positive or non-finite pivot or diagonal, and a candidate with a
 *   used pixel joint at Z_k <= 1e-3) keep x, lambda = min(10 lambda, 1e6).  lambda starts at lambda0.
 * In/out: pose48 (N,48), trans (N,3).  Out: cost (N,2) = C at the input and at the result; status (N) int32 = accepted steps, or -1 for a
 * problem with fewer than 4 used pixel joints, or -2 for one with a used pixel joint at Z_k <= 1e-3 at its input; neither is solved
 * (their pose48 / trans rows are not written; with -2 cost is C as evaluated there).  Optional out (NULL allowed): proj (N,21,3) = (u, v, d)
 * and jac (N,63,51) at the final x; a joint that is neither pixel-used nor in front (Z_k <= 1e-3) has u = v = 0 and zero u / v rows.
 * iters == 0 evaluates cost, proj and jac at the input and writes neither pose48 nor trans.
 * HARP_ERR_ARG before any launch: m, opt, betas, cam, targets, pose48, trans, cost or status NULL; N <= 0; iters < 0; lambda0,
 * pose_prior_weight or z_prior_weight negative or not finite; focal not positive and finite; S <= 0; z_prior NULL with z_prior_weight != 0.
 * harp_mano_reproj_ik_frames_per_block: the problems one workgroup solves (tests size their batches around it). */
typedef struct harp_reproj_ik_options {
  int iters;
  float lambda0;            /* 1e-3 */
  float pose_prior_weight;  /* px^2 / rad^2 */
  float z_prior_weight;     /* px^2 / m^2 */
  int betas_per_frame;      /* 0: betas (10,); otherwise betas (N,10) */
  int cam_per_frame;        /* 0: cam (3,); otherwise cam (N,3) */
  float focal;              /* pixels */
  int S;                    /* image size, pixels */
} harp_reproj_ik_options;
int harp_mano_reproj_ik_frames_per_block(void);
int harp_mano_reproj_ik(const harp_mano_model* m, const float* betas, const float* cam, const float* targets, const float* weights,
                        const float* depth_weights, const float* prior, const float* z_prior, int N, const harp_reproj_ik_options* opt,
                        float* pose48, float* trans, float* cost, int32_t* status, float* proj, float* jac, hipStream_t stream);

/* ---- batched 2.5-D reprojection IK on the joint tree: image keypoints -> SMPL-X arm rows (csrc/arm_reproj_ik.hip; playback
 * Motion.from_arm_image_keypoints) ----
 * Nothing in the reference does this.  The model inverted is harp_lbs_tree_fwd's, seen through the camera and pixel centres of
 * harp_mano_reproj_ik.  N independent Levenberg-Marquardt solves in one launch (one kernel node), forward only, no workspace, no
 * allocation, no synchronisation, no atomics, fixed summation order (capturable; a repeated call gives the same bits).  Unknowns per
 * problem x = [rot 3 | wrist 3 | pose 45 | trans 3]: x[0..51) is the problem's row of in_pose (N,17,3) and x[51..54) its trans, exactly as
 * harp_arm_ik takes them.  Given: betas (10,) for all problems, or (N,10) with betas_per_frame != 0 (the model's other NB - 10
 * coefficients are zero); cam (3,), or (N,3) with cam_per_frame != 0; focal and S (the image is S x S pixels).
 *   j(x) (n_out,3) metres = harp_arm_ik's joints, n_out = n_joints_out <= 22 (the arm: the wrist, the five fingers root to tip, the elbow
 *   as row 21), rows from the model's joint_src.
 *   Z_k = j_k.z + t_z, t_z = 2 focal / (S cam0 + 1e-9);   u_k = S/2 + focal (j_k.x + cam1) / Z_k;   v_k = S/2 + focal (j_k.y + cam2) / Z_k;
 *   d_k = j_k.z - j_0.z: harp_mano_reproj_ik's convention (the centre of column i at u = i + 0.5), over n_out rows, the elbow's d included.
 *   C(x) = sum_k w_k [(u_k - U_k)^2 + (v_k - V_k)^2] + sum_{k>=1} wz_k (d_k - D_k)^2 + pose_prior_weight sum_i (pose_i - prior_i)^2
 *          + wrist_prior_weight sum_i (wrist_i - wrist_prior_i)^2 + z_prior_weight (trans_z - z_prior)^2;
 *   targets (N,n_out,3) = (U, V, D): pixels, pixels, metres; weights (N,n_out) or NULL (ones); depth_weights (N,n_out) or NULL (no depth
 *   rows; the wrist's own entry is never used); prior (N,45) or NULL (zeros: the model's mean pose); wrist_prior (N,3) or NULL (zeros);
 *   z_prior (N) or NULL (then z_prior_weight must be 0).  The weights are in px^2 per squared unit of their residual.  A joint's PIXEL rows
 *   are used when w_k > 0 and U_k, V_k are finite; its DEPTH row when k >= 1, wz_k > 0 and D_k is finite; an unused entry never enters
 *   arithmetic.
 *   solve_wrist == 0: the wrist row of in_pose is read and never written; its three columns are FROZEN as in harp_arm_ik (A_ii = 1, zeros
 *   elsewhere in its row and column, g_i = 0: its step is exactly 0).
 *   Iteration, exactly `iters` times, harp_mano_ik's: J = the exact 3 n_out x 54 derivative of the rows (u, v, d) at x; A = J^T W J + P,
 *   g = J^T W r + P (x - x_prior), P = the three prior weights on the 45 pose, 3 wrist and trans_z diagonals; (A + lambda diag A) d = -g by
 *   a Cholesky factorisation of the matrix scaled from both sides by 1 / sqrt(A_ii (1 + lambda)); x' = x + d; C(x') < C(x): accept,
 *   lambda = max(0.1 lambda, 1e-9); otherwise (a NaN included, a non-positive or non-finite pivot or diagonal, and a candidate with a used
 *   pixel joint at Z_k <= 1e-3) keep x, lambda = min(10 lambda, 1e6).  lambda starts at lambda0.
 * In/out: in_pose (N,17,3) (the wrist row only when solve_wrist), trans (N,3).  Out: cost (N,2) = C at the input and at the result; status
 * (N) int32 = accepted steps; -1 for a problem with fewer than 4 used pixel joints; -2 (cost 0, nothing else written) when the model's tree
 * is not one the kernel's tables hold, by harp_arm_ik's rule; -3 for a problem with a used pixel joint at Z_k <= 1e-3 at its input (cost is
 * C as evaluated there).  None of the three is solved: their in_pose / trans rows are not written.  Optional out (NULL allowed), at the
 * final x: proj (N,n_out,3) = (u, v, d) and jac (N,3 n_out,54), always all 54 columns; a joint that is neither pixel-used nor in front
 * (Z_k <= 1e-3) has u = v = 0 and zero u / v rows.  The elbow's rows in the 48 wrist and finger columns, and d d_k / d trans, are exactly 0.
 * iters == 0 evaluates cost, proj and jac at the input and writes neither in_pose nor trans.
 * HARP_ERR_ARG before any launch: m, opt, betas, cam, targets, in_pose, trans, cost or status NULL; N <= 0; iters < 0; lambda0 or a prior
 * weight negative or not finite; focal not positive and finite; S <= 0; z_prior NULL with z_prior_weight != 0; n_joints_out outside
 * 1..HARP_ARM_IK_MAX_JOINTS; center_joint outside [0, NJ); n_pose_in != 17; NB < 10, NB > 32 or NJ > 64.
 * harp_arm_reproj_ik_frames_per_block: the problems one workgroup solves (tests size their batches around it). */
typedef struct harp_arm_reproj_ik_options {
  int iters;
  float lambda0;            /* 1e-3 */
  float pose_prior_weight;  /* px^2 / rad^2 */
  float wrist_prior_weight; /* px^2 / rad^2 */
  float z_prior_weight;     /* px^2 / m^2 */
  int solve_wrist;          /* 0: the wrist row of in_pose given and frozen */
  int betas_per_frame;      /* 0: betas (10,); otherwise betas (N,10) */
  int cam_per_frame;        /* 0: cam (3,); otherwise cam (N,3) */
  float focal;              /* pixels */
  int S;                    /* image size, pixels */
} harp_arm_reproj_ik_options;
int harp_arm_reproj_ik_frames_per_block(void);
int harp_arm_reproj_ik(const harp_tree_model* m, const float* betas, const float* cam, const float* targets, const float* weights,
                       const float* depth_weights, const float* prior, const float* wrist_prior, const float* z_prior, int N,
                       const harp_arm_reproj_ik_options* opt, float* in_pose, float* trans, float* cost, int32_t* status, float* proj,
                       float* jac, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HARP_HIP_H */
