/* rt_abi.h -- C ABI of the MI355X render path (librt_mi355x.so).
 *
 * This is the drop-in boundary for the reference's one hot path: the kernel
 * launches its host scene functions make (src/main.cu:685-732 and the same
 * pattern in every scene function).  The reference has no FFI layer; what a
 * maintainer would bind is exactly this set of entry points, each of which
 * replaces a group of reference launches/runtime calls:
 *
 *   rt_init / rt_shutdown       cudaDeviceSetLimit x2 (main.cu:665-666), cudaDeviceReset (main.cu:743)
 *   rt_scene_create             cudaMalloc(d_list|d_world|d_camera) + create_world_*<<<1,1>>>
 *                               (main.cu:688-697); the device-heap object graph becomes flat arrays
 *   rt_render                   cudaMallocManaged(fb) + cudaMalloc(d_rand_state) + render_init<<<>>> +
 *                               render<<<>>> + both syncs (main.cu:676-680, 702-709)
 *   rt_scene_destroy            free_world<<<1,1>>> + cudaFree x5 (main.cu:732-740)
 *   rt_strerror / rt_last_hip_error   checkCudaErrors (main.cu:23-35), minus the exit(99)
 *
 * Plain C, plain pointers and sizes.  No C++ types, no torch types.
 * Caller owns every rt_scene_desc array and the framebuffer; the library owns
 * all device memory behind rt_scene*.  Not re-entrant per rt_scene*.
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int rt_status;
enum {
    RT_OK = 0,
    RT_ERR_INVALID = 1,      /* bad argument / malformed scene description */
    RT_ERR_NO_DEVICE = 2,    /* no gfx950 device visible */
    RT_ERR_HIP = 3,          /* a HIP runtime call failed; see rt_last_hip_error() */
    RT_ERR_UNSUPPORTED = 4   /* scene uses a nesting the kernels do not implement */
};

/* ---- flattened scene (what create_world_* builds with device-side new) ---- */

/* primitive reference = (kind << 28) | index into that kind's array */
enum { RT_PRIM_SPHERE = 0, RT_PRIM_QUAD = 1, RT_PRIM_BOX = 2, RT_PRIM_INSTANCE = 3, RT_PRIM_MEDIUM = 4 };
#define RT_PRIM_REF(kind, index) ((int32_t)(((uint32_t)(kind) << 28) | (uint32_t)(index)))
#define RT_PRIM_KIND(ref) ((int)(((uint32_t)(ref)) >> 28))
#define RT_PRIM_INDEX(ref) ((int)(((uint32_t)(ref)) & 0x0FFFFFFFu))

/* bvh_node (bvh.cuh:9-116) flattened in depth-first pre-order ("threaded"):
 * a node whose box is hit continues at index+1 (its left child) unless it is a
 * leaf; a node whose box is missed, and a finished leaf, continue at `skip`.
 * prim < 0: internal node.  Every object sits in its own leaf node whose box
 * is the object's box (the reference's n==1 node, bvh.cuh:38-43).
 * n_nodes == 0 is a legal description: an empty world, every ray misses and the
 * frame is the background (one ray per sample). */
typedef struct rt_node {
    float bmin[3];
    int32_t skip;
    float bmax[3];
    int32_t prim;
} rt_node; /* 32 B */

/* sphere (sphere.cuh:10-102): centre c(t) = c0 + t*vel, vel = 0 when static */
typedef struct rt_sphere {
    float c0[3];
    float radius;
    float vel[3];
    int32_t mat;
} rt_sphere; /* 32 B */

/* quad (quad.cuh:11-91) with its constructor-derived fields precomputed */
typedef struct rt_quad {
    float Q[3];
    float D;
    float u[3];
    int32_t mat;
    float v[3];
    float pad0;
    float w[3];
    float pad1;
    float n[3];
    float pad2;
} rt_quad; /* 80 B */

/* compound6 (quad.cuh:94-143): six consecutive quads, scan order = array order */
typedef struct rt_box {
    int32_t first_quad;
} rt_box;

/* translate(rotate_y(child)) (hittable.cuh:40-149); either half may be absent */
enum { RT_INST_ROTATE_Y = 1, RT_INST_TRANSLATE = 2 };
typedef struct rt_instance {
    float sin_t, cos_t;
    float offset[3];
    int32_t child;  /* prim ref: sphere, quad or box */
    int32_t flags;
    int32_t pad;
} rt_instance; /* 32 B */

/* constant_medium (constant_medium.cuh:16-80) */
typedef struct rt_medium {
    int32_t boundary; /* prim ref: sphere, quad, box or instance */
    float neg_inv_density;
    int32_t mat;      /* isotropic phase function */
    int32_t pad;
} rt_medium; /* 16 B */

enum { RT_MAT_LAMBERTIAN = 0, RT_MAT_METAL = 1, RT_MAT_DIELECTRIC = 2, RT_MAT_DIFFUSE_LIGHT = 3, RT_MAT_ISOTROPIC = 4 };
/* material.cuh:62-201.  tex < 0: `albedo` is the (solid) colour. */
typedef struct rt_material {
    int32_t kind;
    int32_t tex;
    float fuzz; /* metal, already clamped to <= 1 (material.cuh:97) */
    float ior;  /* dielectric */
    float albedo[3];
    float pad;
} rt_material; /* 32 B */

enum { RT_TEX_SOLID = 0, RT_TEX_CHECKER = 1, RT_TEX_IMAGE = 2, RT_TEX_NOISE = 3, RT_TEX_NOODLE = 4, RT_TEX_FELT = 5, RT_TEX_UV_OFFSET = 6 };
/* texture.cuh:16-164.
 * checker: a/b = even/odd texture index, scale = 1/scale.
 * image: a = byte offset into `images`, b = width, c = height (RGB8).
 * noise: scale.
 * noodle (texture.cuh:84-103): scale = k, p[6] = A, p[7] = f, a = octaves, p[3..5] = unit direction,
 *   color = noodle colour, p[0..2] = gap colour.
 * felt (texture.cuh:109-148): color = base, scale = mottling scale, p[0] = mottling amount, p[1] = fibre scale,
 *   p[2] = fibre amount.
 * uv_offset (texture.cuh:151-164): a = wrapped texture, scale = du (turns), p[0] = dv. */
typedef struct rt_texture {
    int32_t kind;
    int32_t a, b;
    float scale;
    float color[3];
    int32_t c;
    float p[8];
} rt_texture; /* 64 B */

/* camera (camera.cuh:18-79) after init() */
typedef struct rt_camera {
    float origin[3];
    float lower_left_corner[3];
    float horizontal[3];
    float vertical[3];
    float u[3];
    float v[3];
    float lens_radius;
    float pad;
    double time0, time1;
} rt_camera;

typedef struct rt_scene_desc {
    const rt_node* nodes;         int32_t n_nodes;
    const rt_sphere* spheres;     int32_t n_spheres;
    const rt_quad* quads;         int32_t n_quads;
    const rt_box* boxes;          int32_t n_boxes;
    const rt_instance* instances; int32_t n_instances;
    const rt_medium* media;       int32_t n_media;
    const rt_material* materials; int32_t n_materials;
    const rt_texture* textures;   int32_t n_textures;
    const uint8_t* images;        size_t image_bytes;
    rt_camera camera;
} rt_scene_desc;

/* ---- one frame (the arguments of render<<<>>>, main.cu:107-109) ---- */
typedef struct rt_frame_desc {
    int32_t nx, ny;          /* full image size; pixel_index = j*nx + i, row 0 = bottom (main.cu:115) */
    int32_t ns;              /* samples per pixel */
    float gamma;             /* 1.0 = identity (main.cu:39) */
    float background[3];
    int32_t use_gradient_bg;
    uint64_t seed_base;      /* per-pixel seed = seed_base + pixel_index (main.cu:104: 1984) */
    /* Row partition for multi-GPU runs: the image is cut into tiles of
     * `tile_rows` rows; this call renders tiles tile_first, tile_first +
     * tile_stride, ...  The output buffer is compact: local row k holds global
     * row rt_local_to_global_row(k).  Whole frame: tile_rows = ny,
     * tile_first = 0, tile_stride = 1. */
    int32_t tile_rows, tile_first, tile_stride;
    int32_t reserved;
} rt_frame_desc;

typedef struct rt_stats {
    uint64_t rays;           /* world->hit calls from color() (main.cu:57) */
    uint64_t samples;        /* primary rays */
    double ms_render;        /* device time of the render kernel, HIP events on the launch stream */
    int32_t local_rows;      /* rows written by this call */
    int32_t kernel_variant;  /* which specialisation ran */
    int32_t workgroups, threads_per_group, lds_bytes, reserved;
} rt_stats;

typedef struct rt_scene rt_scene;

rt_status rt_init(int device_ordinal);
rt_status rt_shutdown(void);
const char* rt_strerror(rt_status s);
int rt_last_hip_error(void);            /* hipError_t of the last failing call, 0 if none */
const char* rt_last_error_detail(void); /* "file:line 'expr'" of the last failure, like main.cu:28-29 */

rt_status rt_scene_create(const rt_scene_desc* desc, rt_scene** out);
rt_status rt_scene_destroy(rt_scene* scene);

/* The traversal array behind a scene.  rt_scene_create keeps the reference's depth-first tree and, beside it, the array
 * the render kernels walk: the same leaves in the same order, with the interior nodes whose box test does not pay
 * removed (option "bvh_collapse", read at creation; results are bit-identical either way).  Reports the two
 * node counts and the expected box tests per ray before / after on the calibration frame (0 when nothing was removed). */
rt_status rt_scene_walk_info(const rt_scene* scene, int32_t* nodes_reference, int32_t* nodes_walked,
                             double* tests_before, double* tests_after);
/* The planner behind it, host only (no device needed): the walk array for `nodes` given per-node counts of passing box
 * tests (`pass`, null = proportional to box surface area) out of `root_visits` rays.  out/cap may be null/0. */
rt_status rt_plan_walk_array(const rt_node* nodes, int32_t n, const double* pass, double root_visits, rt_node* out, int32_t cap,
                             int32_t* n_out, double* tests_before, double* tests_after);

/* Another hierarchy over the same leaves, host only: the leaves of `nodes` (its single-object nodes, boxes and order
 * untouched) under a binary tree whose interior boxes are the union of their leaves' boxes; method 0 = top-down by
 * surface-area cost, 1 = bottom-up (merge the neighbouring groups with the smallest union).  Any such tree gives the
 * reference's results; rt_scene_create (bvh_collapse = 3) measures both beside the reference's tree and
 * walks whichever needs the fewest box tests.  out holds up to cap nodes; *n_out = 2 * leaves - 1. */
rt_status rt_regroup_leaves(const rt_node* nodes, int32_t n, int32_t method, rt_node* out, int32_t cap, int32_t* n_out);

/* Number of rows a frame description assigns to this call, and the mapping
 * from a compact local row to its global row. */
int32_t rt_frame_local_rows(const rt_frame_desc* f);
int32_t rt_local_to_global_row(const rt_frame_desc* f, int32_t local_row);

/* render_init + render (main.cu:96-133) for the rows this call owns.
 * fb: float RGB, rt_frame_local_rows(f) * nx * 3 elements.  fb_on_device != 0:
 * fb is device memory and the kernel writes it directly; otherwise it is host
 * memory and the library copies the rows back.  stream: a hipStream_t (0 =
 * default stream).  The call returns after the frame is complete when
 * `blocking` != 0; otherwise work is only enqueued on `stream` and
 * stats->ms_render / rays are valid after rt_frame_finish(). */
rt_status rt_render(rt_scene* scene, const rt_frame_desc* f, float* fb, int fb_on_device,
                    void* stream, int blocking, rt_stats* stats);
rt_status rt_frame_finish(rt_scene* scene, rt_stats* stats);

/* ---- batched ray queries against a scene resident on the device ----
 * The render kernels' BVH walk and leaf tests (the reference's bvh_node::hit, bvh.cuh:95-106, and its objects' hit
 * functions), asked for caller-supplied rays.  For a ray with the default window (tmin = 0.001f, tmax null) the closest t
 * is bit-identical to what the reference's world->hit returns for it (main.cu:57), media included: constant_medium draws
 * its uniform from a hash of the ray, so its result is a function of the ray alone.
 *
 * Pointers: every pointer in the batch is device (or managed) memory of the scene's device, 4-byte aligned.  Each
 * non-null one is checked with hipPointerGetAttributes before anything is launched; a host pointer, an unregistered
 * pointer or one on another device is RT_ERR_INVALID.
 * Arguments: a null scene or batch, n < 0, a non-finite tmin, an unknown mode or a wrong set of outputs for the mode is
 * RT_ERR_INVALID; these checks run before any HIP call and before the scene is looked at, and rt_last_error_detail()
 * names the one that failed.
 * Window: each object applies (tmin, tmax) as the reference's hit function does: a sphere accepts tmin < t < tmax, a quad
 * (and a box face) tmin <= t <= tmax, a medium clamps its interval to [tmin, tmax] (so may return t == tmax).  tmax is
 * per ray (null = FLT_MAX); a ray whose tmax is NaN is a miss.  So is a ray with a NaN or infinite component in its origin,
 * direction or time: it is decided before the walk (the reference's quad and medium tests would accept a NaN t).
 * Stream: the work is enqueued on `stream` (a hipStream_t, 0 = default stream), like rt_render; with `blocking` != 0 the
 * call returns when every output is written.
 * Shared state: none.  The call reads only the scene's immutable device arrays and the process options; it touches none
 * of the per-frame resources of rt_render (counters, events, the pending frame, the tier stream).  A trace may therefore
 * run while a non-blocking rt_render of the same scene is still pending on another stream.  Options (rt_set_option):
 * "trace_lds" -1 = auto (the largest LDS mode whose image still leaves at least 3/4 of the workgroups per CU that the
 * scene-through-L1/L2 mode gets), 0 = scene through L1/L2, 1 = nodes in LDS, 2 = nodes and spheres in LDS (a forced mode
 * that does not fit falls back to the largest that does); "trace_tree" 1 = the walk array, 0 = the reference's full tree.
 * Neither changes a result. */
enum { RT_TRACE_CLOSEST = 0, RT_TRACE_ANY = 1 };
typedef struct rt_ray_batch {
    int64_t n;                 /* rays; 0 is a no-op */
    const float* origins;      /* n*3, required */
    const float* directions;   /* n*3, required; not normalised (the reference never normalises) */
    const float* times;        /* n, null = 0 for every ray (moving spheres; the camera's rays carry time0..time1) */
    const float* tmax;         /* n, null = FLT_MAX for every ray; upper end of the window (see Window above) */
    float tmin;                /* lower end of the window; the reference's is 0.001f (main.cu:57); must be finite */
    int32_t mode;              /* RT_TRACE_CLOSEST or RT_TRACE_ANY */
    /* CLOSEST: t_out and prim_out required, the rest optional (null = not written). */
    float* t_out;              /* closest t, FLT_MAX on a miss */
    int32_t* prim_out;         /* resolved leaf as RT_PRIM_REF: sphere, quad (a box face: its quad) or medium; -1 on a miss */
    int32_t* inst_out;         /* instance index the hit went through, -1 if none or on a miss */
    float* point_out;          /* n*3 hit_record p */
    float* normal_out;         /* n*3 hit_record normal as the reference orients it (quad and rotate_y face the ray; medium (1,0,0)) */
    float* uv_out;             /* n*2 hit_record u, v (sphere: get_sphere_uv of the object-space normal, sphere.cuh:42-49; medium 0, 0) */
    int32_t* mat_out;          /* n material index */
    /* ANY: hit_out only, required; every CLOSEST output must be null. */
    uint8_t* hit_out;          /* 1 if some leaf is accepted in the window, else 0 */
    /* A miss writes t = FLT_MAX, prim = inst = mat = -1 and zeros to point, normal and uv. */
} rt_ray_batch;
rt_status rt_trace_rays(rt_scene* scene, const rt_ray_batch* batch, void* stream, int blocking);

/* ---- radiance queries: path-traced colour along caller-supplied rays ----
 * The renderer's color() loop (main.cu:52-94: bounces, materials, textures, media, the 50-bounce cut) for rays the caller
 * chose instead of the one thin-lens camera of rt_scene_desc: panoramic or orthographic views, light probes, lightmap texels.
 *
 * Contract per ray i, with seed_i = seeds[i] (seeds null: seed_base + i): rgb_out[i] is bit for bit what rt_render writes for
 * the single pixel of a 1 x 1 frame with `ns` samples, gamma 1, the batch's background and seed_base = seed_i, of a scene
 * whose camera is the degenerate one that sends every sample along this ray -- horizontal = vertical = 0, lens_radius = 0,
 * origin = o, time0 = time1 = tm and lower_left_corner chosen so that fl(lower_left_corner - o) = d -- and rays_out[i] is
 * that frame's ray count (world->hit calls).  Spelled out: one XORWOW chain is seeded with seed_i; each of the ns samples
 * first draws and discards what a render sample draws before its path (two jitter uniforms, the lens-disk rejection loop at
 * two uniforms per turn, one shutter uniform), then runs color() on (o, d, tm); the sum is scaled as the frame's pixel is, by
 * (float)(1.0 / (double)(float)ns).  The camera draws are kept although they select nothing: they make a query equal to a
 * pixel of rt_render, and that identity is what makes every query checkable against the renderer and its CPU oracle.
 * A ray with a NaN or infinite component in its origin, direction or time, or with an all-zero direction, gets rgb = 0 and
 * rays = 0; it is decided before the walk and consumes no draws.
 *
 * Pointers, arguments, stream and shared state: the contract of rt_trace_rays.  Every pointer is device (or managed) memory
 * of the scene's device, 4-byte aligned (seeds: 8-byte), checked with hipPointerGetAttributes before anything is launched.
 * A null scene or batch, n < 0, ns outside [1, 1 << 20] or a missing required pointer (origins, directions, rgb_out) is
 * RT_ERR_INVALID; these checks run before any HIP call and before the scene is looked at, and rt_last_error_detail() names
 * the one that failed.  The work is enqueued on `stream`; with `blocking` != 0 the call returns when every output is
 * written.  The call touches none of rt_render's per-frame resources, so it may run beside a pending non-blocking
 * rt_render of the same scene.  Option "radiance_lds": -1 = auto ("trace_lds"'s rule), 0 = scene through L1/L2, 1 = nodes
 * in LDS, 2 = nodes and spheres in LDS (a forced mode that does not fit falls back to the largest that does); it changes
 * no result. */
typedef struct rt_radiance_batch {
    int64_t n;                 /* rays; 0 is a no-op */
    const float* origins;      /* n*3, required */
    const float* directions;   /* n*3, required; not normalised */
    const float* times;        /* n, null = 0 for every ray */
    const uint64_t* seeds;     /* n, null = seed_base + i */
    uint64_t seed_base;
    int32_t ns;                /* samples per ray, 1 <= ns <= 1 << 20 */
    float background[3];       /* the miss term, as rt_frame_desc */
    int32_t use_gradient_bg;
    int32_t reserved;
    float* rgb_out;            /* n*3, required */
    uint32_t* rays_out;        /* n, optional (null = not written): the world->hit calls of each query */
} rt_radiance_batch; /* 88 B */
rt_status rt_radiance_rays(rt_scene* scene, const rt_radiance_batch* batch, void* stream, int blocking);

/* ---- feature buffers: per-pixel albedo, normal, depth, coverage and ids of a frame's first hits ----
 * What a denoiser, a compositor, a picker or an edge-aware upscaler needs beside a noisy frame (rt_render at few samples,
 * rt_render_adaptive) of the same camera.
 *
 * The feature pass of a frame runs, per pixel, one XORWOW chain seeded seed_base + pixel_index, with rt_render's pixel
 * indexing (pixel_index = global_row * nx + column) and row partition.  Each of the ns samples draws what a render sample
 * draws before its path -- two jitter uniforms, camera_get_ray's lens-disk loop at two uniforms per turn, its shutter
 * uniform -- and nothing else; its primary ray is walked with the render's window (0.001, FLT_MAX) (world->hit, main.cu:57)
 * and the hit record is resolved as rt_trace_rays resolves it.  Sample s of a pixel is therefore the primary ray rt_render
 * would send if no path ever consumed a draw; sample 0 is exactly rt_render's first primary ray of that pixel.
 *
 * Per sample:
 *   albedo  lambertian or isotropic hit: the material's texture value at (u, v, p), or its `albedo` when tex < 0; metal:
 *           `albedo`; dielectric: (1, 1, 1); diffuse light: what it emits there; miss: the frame's miss term as rt_render
 *           computes it (background, or the gradient of the ray).  The first hit only: no specular bounce is followed.
 *   normal  the hit record's normal, oriented as normal_out of rt_trace_rays (against the ray for quads and rotated
 *           instances, outward for spheres); a constant medium gives (1, 0, 0); a miss gives 0.
 *   depth   the hit record's t: the ray PARAMETER, not a distance -- directions are not normalised, so the distance is
 *           t * |d|.  A miss gives 0.
 *   alpha   1 on a hit, 0 on a miss.
 * Per pixel, each float output is the sum over the samples in sample order, per channel, plain sum = sum + x in binary32
 * with no contraction, multiplied by (float)(1.0 / (double)(float)ns) -- store_pixel's factor.  No gamma is applied:
 * f->gamma is ignored.  prim / inst / mat are sample 0's prim_out / inst_out / mat_out as rt_trace_rays defines them, -1 on
 * a miss.
 *
 * The identity that makes every output checkable: in the "emissive twin" of a scene -- every material turned into
 * RT_MAT_DIFFUSE_LIGHT; lambertian, isotropic and light keep tex and albedo, metal takes tex = -1, dielectric tex = -1 and
 * albedo = (1, 1, 1) -- every path ends at its first hit and consumes no draw, so `albedo` equals, bit for bit, the frame
 * rt_render gives for the twin at gamma 1 with the same ns, seed_base, background and partition.
 *
 * f supplies nx, ny, ns, background, use_gradient_bg, seed_base and the tile partition.  Every pointer of rt_aov_desc is
 * optional, at least one is non-null; the buffers hold compact local rows like fb (rt_frame_local_rows(f) rows).  What no
 * requested output needs is not computed (no texture without albedo).  buffers_on_device != 0: device (or managed) memory
 * of the scene's device, 4-byte aligned, checked with hipPointerGetAttributes before anything is launched; the work is
 * enqueued on `stream` and with `blocking` != 0 the call returns when every output is written (rt_trace_rays' rules).
 * buffers_on_device == 0: host memory; the library stages the outputs in device memory of the call's own, copies them back
 * and returns when they are complete, whatever `blocking` says.  A null scene, f or a, every output null, non-positive nx, ny
 * or ns, a frame of 2^31 pixels or more or a bad row partition (rt_render's checks) is RT_ERR_INVALID; these checks run
 * before any HIP call and before the scene is looked at, and rt_last_error_detail() names the one that failed.  The call
 * uses none of rt_render's per-frame resources and no shared state, so it may run beside a pending non-blocking rt_render
 * of the same scene on another stream.  Option "aov_lds": the meaning and auto rule of "trace_lds"; it changes no result. */
typedef struct rt_aov_desc {
    float* albedo;             /* rows*nx*3 */
    float* normal;             /* rows*nx*3 */
    float* depth;              /* rows*nx */
    float* alpha;              /* rows*nx */
    int32_t* prim;             /* rows*nx each */
    int32_t* inst;
    int32_t* mat;
} rt_aov_desc; /* 56 B */
rt_status rt_render_aov(rt_scene* scene, const rt_frame_desc* f, const rt_aov_desc* a, int buffers_on_device, void* stream, int blocking);

/* ---- feature buffers through mirrors and glass: the first non-specular surface of every sample ----
 * rt_render_aov stops at the first hit, so a glass ball has albedo (1, 1, 1) and a mirror its tint, and both have their own
 * normal: nothing of what is seen through or in them.  rt_render_aov_through follows a deterministic specular chain from
 * each primary ray -- the mirror direction of a metal, the refracted direction of a dielectric (the mirror direction under
 * total internal reflection) -- and reports the surface where the chain ends: what a denoiser asks its caller for.
 *
 * Everything of rt_render_aov's contract holds: the pixel's XORWOW chain and its draws, pixel indexing, row partition, the
 * buffers and their rules, the checks before any HIP call, the stream rules, no shared state.  The specular chain consumes no
 * draw, so sample s of a pixel starts from exactly the primary ray rt_render_aov uses.  Per sample, with ray 0 the primary
 * ray (o0, d0, tm) and k = 0:
 *   Walk.  Ray k is walked with the window (0.001, FLT_MAX) and its hit resolved as rt_trace_rays resolves it.
 *   Terminal events.  The chain ends at: a miss; a hit on a lambertian, isotropic or light material (a constant medium's
 *     material included); a metal with fuzz > fuzz_limit; any hit once k == max_bounces; a followed metal whose mirror
 *     direction r has dot(n, r) <= 0.
 *   Follow.  Otherwise the hit is followed: ray k + 1 is (p, d', tm), p the hit record's point, n its normal as normal_out
 *     orients it, and k = k + 1.
 *   d'.  All binary32, every written operation rounded once, nothing contracted into an FMA, sums left to right as written;
 *     only + - * / sqrt and comparisons occur.  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.  u = d / sqrt(dot(d, d)), three
 *     divisions.
 *       metal       c = dot(u, n);  r = u - (2 c) n per component.  dot(n, r) <= 0: the hit is terminal and the tint stays.
 *                   Else d' = r and the chain's tint, (1, 1, 1) at the start, is multiplied per channel by the
 *                   material's albedo.
 *       dielectric  dn = dot(d, n);  dn > 0: m = -n, e = ior;  else m = n, e = 1 / ior.  dt = dot(u, m);
 *                   disc = 1 - (e e) (1 - dt dt).  disc > 0: d' = e (u - dt m) - sqrt(disc) m per component (refraction);
 *                   else d' = u - (2 dot(u, n)) n (total internal reflection).  The tint is unchanged.
 *   Terms of the sample, from the terminal event:
 *     albedo   tint times, per channel, rt_render_aov's albedo of the terminal hit -- or, on a miss, its miss term of the
 *              last ray.
 *     normal   the terminal hit's normal; 0 on a miss.
 *     alpha    1 on a terminal hit, 0 on a miss.
 *     depth    on a terminal hit, in the PRIMARY ray's parameter: t0 when nothing was followed (k = 0), else
 *              t0 + ((t1 + t2) + ... + tk) / sqrt(dot(d0, d0)), t_j the hit's t along ray j; 0 on a miss.
 *     through  1 if k >= 1, else 0.
 *   Per pixel each float output (albedo, normal, depth, alpha, through) is the sum of the terms in sample order, scaled by
 *   (float)(1.0 / (double)(float)ns), as rt_render_aov does.  prim / inst / mat are sample 0's terminal hit (-1 on a terminal
 *   miss) and bounces is sample 0's k, whatever ended its chain.
 * With max_bounces = 0 every output of rt_aov_desc is bit for bit rt_render_aov's (through = 0, bounces = 0).
 *
 * A null t, max_bounces outside 0..16, a non-finite or negative fuzz_limit, or every output of a and t null is
 * RT_ERR_INVALID beside rt_render_aov's checks; all run before any HIP call and before the scene is looked at, and
 * rt_last_error_detail() names the one that failed.  Option "aov_through_lds": the meaning and auto rule of "trace_lds"; it
 * changes no result. */
typedef struct rt_aov_through_desc {
    int32_t max_bounces;       /* 0..16; 0 = rt_render_aov */
    float fuzz_limit;          /* finite, >= 0: a metal is followed iff its fuzz <= fuzz_limit */
    float* through;            /* rows*nx or null: share of the pixel's samples that followed at least one bounce */
    int32_t* bounces;          /* rows*nx or null: sample 0's number of followed bounces */
} rt_aov_through_desc; /* 24 B */
rt_status rt_render_aov_through(rt_scene* scene, const rt_frame_desc* f, const rt_aov_desc* a, const rt_aov_through_desc* t,
                                int buffers_on_device, void* stream, int blocking);

/* ---- denoiser: an edge-avoiding a-trous wavelet filter guided by the feature buffers ----
 * rt_denoise filters a noisy linear frame (rt_render or rt_render_adaptive at gamma 1) with a 5x5 B3-spline kernel whose
 * taps are spread 2^k pixels apart in iteration k and weighted down across edges of the normal, the depth and the colour.
 * It takes no scene and runs on the device the last rt_init selected.
 *
 * The numerical contract.  All arithmetic is binary32, every written operation is rounded once, nothing is contracted
 * into an FMA, sums run left to right as written; only + - * /, max, abs and comparisons occur (max returns the other operand
 * when one is a NaN); subnormal results are kept, never flushed to zero.  Images are whole frames of ny x nx pixels,
 * row-major, row 0 at the bottom, as rt_render writes an unpartitioned frame: color (x3) is required; albedo (x3), normal (x3)
 * and depth (x1) are optional and are what rt_render_aov writes.
 *   Prepare.  demodulate != 0: per channel a = max(albedo, 2^-10), x_0 = color / a (a null albedo is then RT_ERR_INVALID);
 *     otherwise x_0 = color.
 *   Iteration k = 0 .. iterations-1, s = 2^k, pixel p = (i, j).  W = 0, S = (0, 0, 0).  For dy = -2..2 (outer), dx = -2..2
 *     (inner), q = (i + s dx, j + s dy); a q outside the image is skipped.  w = H[dy] H[dx], H = {1/16, 1/4, 3/8, 1/4, 1/16}
 *     (every product is exact).  The centre tap (dx = dy = 0) takes no further factor, so W >= 9/64 whatever the guides
 *     hold.  Every other tap multiplies w by these factors, in this order (w = w * factor); a factor that is off is not applied:
 *       normal  (normal non-null and normal_sharpness = m in 1..10; 0 = off):
 *               d = (Np.x Nq.x + Np.y Nq.y) + Np.z Nq.z;  d = max(d, 0);  then d = d d, m times (the exponent is 2^m);
 *               the factor is d.
 *       depth   (depth non-null and sigma_depth > 0):
 *               den = sigma_depth max(Zp, Zq) + 1e-20f;  r = |Zp - Zq| / den;  t = max(1 - r, 0);  the factor is t t.
 *       colour  (sigma_color > 0), on x_k:  sp = (xp.r + xp.g) + xp.b, sq likewise;  d1 = (|dr| + |dg|) + |db|, the channel
 *               differences xp - xq;  den = (sigma_color 2^-k) ((sp + sq) + color_floor);  r = d1 / den;
 *               t = max(1 - r, 0);  the factor is t t.
 *     Then W = W + w and, per channel, S.ch = S.ch + w xq.ch.  After the 25 taps x_{k+1}(p).ch = S.ch / W.
 *   Finish.  out = x_K a per channel when demodulating, else x_K.  No gamma is applied.
 * tests/denoise_expect.py restates this in NumPy float32; the device result equals it bit for bit.
 * Inputs are expected to be finite.  A NaN, an infinity or a negative depth or albedo changes nothing beyond the pixels within
 * reach of it (2 (2^K - 1) pixels each way); within reach the result is what the rules above give in IEEE 754 arithmetic with
 * that max -- a NaN where the restatement has one (its sign and payload are not specified), the restatement's bits elsewhere.
 * So a NaN depth or normal takes its taps' weight away (max(1 - NaN, 0) = 0) and a non-finite colour spreads as NaN (0 x NaN).
 * No value of any input makes the call fault: no address depends on pixel data.  (tests/test_filter_domain.py)
 *
 * Parameters (anything else is RT_ERR_INVALID): iterations 1..8; nx, ny >= 1 and nx ny < 2^31; normal_sharpness 0..10;
 * sigma_depth and sigma_color each 0 or finite in [1e-6, 1e6]; color_floor finite and > 0 when sigma_color > 0; color and
 * out non-null.  out may be exactly color (in place); any other overlap among the buffers and the workspace is
 * RT_ERR_INVALID where the host can see it and undefined otherwise.
 *
 * Buffers: rt_render_aov's rules.  buffers_on_device != 0: every non-null buffer (and the workspace) is device or managed
 * memory of that device, 4-byte aligned (the workspace 16-byte), checked with hipPointerGetAttributes before anything is
 * launched; the work is enqueued on `stream` and with `blocking` != 0 the call returns when out is written.
 * buffers_on_device == 0: host memory; the library stages the buffers in device memory of the call's own, copies out back
 * and returns when it is complete, whatever `blocking` says; a workspace is then checked for its size and not used.
 * Workspace: rt_denoise_workspace_bytes(nx, ny) bytes of device memory (0 for a bad size) -- two colour images and one
 * guide image of 16-byte records.  A non-null workspace smaller than that is RT_ERR_INVALID.  With a null workspace the
 * library allocates its own and waits before freeing it, whatever `blocking` says; with a caller's workspace and
 * blocking == 0 the call only enqueues.  The argument checks run before any HIP call and rt_last_error_detail() names the
 * one that failed.  The call uses no scene and no shared state, so it may run beside a pending non-blocking rt_render on
 * another stream.  Option "denoise_lds": -1 (auto) = iterations whose taps are at most 4 pixels apart stage their tile and
 * its halo in LDS, the others read their taps through L1/L2; 0 = never stage; 1 = stage wherever the tile fits (taps up to 8
 * apart).  It changes no result. */
typedef struct rt_denoise_desc {
    int32_t nx, ny;
    const float* color;        /* ny*nx*3, linear */
    const float* albedo;       /* ny*nx*3 or null */
    const float* normal;       /* ny*nx*3 or null */
    const float* depth;        /* ny*nx or null */
    float* out;                /* ny*nx*3; may be exactly `color` */
    void* workspace;           /* device memory, or null */
    size_t workspace_bytes;
    int32_t iterations, normal_sharpness, demodulate, reserved;
    float sigma_color, color_floor, sigma_depth, pad;
} rt_denoise_desc; /* 96 B */
size_t rt_denoise_workspace_bytes(int32_t nx, int32_t ny);
rt_status rt_denoise(const rt_denoise_desc* d, int buffers_on_device, void* stream, int blocking);

/* ---- progressive accumulation (the reference writes every pixel's curandState back at the end of render(),
 * main.cu:126, which is what would allow it and what nothing in the reference uses) ----
 * rt_render_window renders samples [sample_begin, sample_end) of every pixel the frame description assigns to the call,
 * continuing from `state` -- device memory made by rt_progressive_state_create for that frame description, opaque to the
 * caller: per pixel the XORWOW state, the colour sum and the rays so far -- and writes to fb the frame averaged over the
 * sample_end samples rendered so far, gamma applied (f->ns is ignored).  sample_begin must be 0 on the first call for a
 * state and the previous call's sample_end afterwards; anything else is RT_ERR_INVALID.  A sequence of windows gives
 * pixels bit-identical to one rt_render with ns = the last sample_end (tests/test_gpu_parity.py); stats->rays counts the
 * window's rays.  Windows run as one launch each (no cost-aware split: a window is usually short). */
rt_status rt_progressive_state_create(rt_scene* scene, const rt_frame_desc* f, void** state);
rt_status rt_progressive_state_destroy(rt_scene* scene, void* state);
rt_status rt_render_window(rt_scene* scene, const rt_frame_desc* f, float* fb, int fb_on_device, void* state,
                           int32_t sample_begin, int32_t sample_end, void* stream, int blocking, rt_stats* stats);

/* ---- adaptive sampling: each pixel stops once its estimate converges ----
 * rt_render_adaptive renders the pixels the frame description assigns to the call (row partition as rt_render; f->ns is
 * ignored) with a per-pixel sample count n_i chosen at the checkpoints c_k = min_spp * 2^k, k = 0..K, where
 * max_spp = min_spp * 2^K.  Parameters: min_spp even and >= 2; 0 <= K <= 16; threshold finite; floor finite and >= 0.
 * At each checkpoint n < max_spp a pixel still active compares its linear average at n samples, a, with its linear average
 * at n/2 samples, h -- each the float the frame would hold at ns = n (resp. n/2) with gamma 1: the colour sum times
 * (float)(1.0 / (double)(float)n), per channel.  In double, left to right, from those floats:
 *     d = |a.x - h.x| + |a.y - h.y| + |a.z - h.z|,   s = a.x + a.y + a.z,
 *     converged  iff  threshold >= 0  and  d <= (double)threshold * (s + (double)floor)
 * (a NaN in d never converges).  A pixel stops at its first converged checkpoint, otherwise at max_spp.
 * Per pixel, with its final count n_i: fb holds what rt_render with ns = n_i and the frame's gamma writes for that pixel
 * (each pixel is one chain seeded by seed_base + its index, so it is the same pixel); spp_out (optional, null = not written;
 * the same kind of memory as fb, compact local rows of nx int32) holds n_i.  stats: rays = the sum of every pixel's rays at
 * its n_i, samples = the sum of the n_i, ms_render = device time from the first pass to the last, reserved = render passes
 * that had work.  So K = 0 gives rt_render at ns = min_spp, and threshold < 0 gives rt_render at ns = max_spp.
 * Passes: [0, min/2) and [min/2, min) over every pixel, then [c_k, c_k+1) over the pixels still active; the call enqueues
 * them on `stream`, reads back one active-pixel count between passes and returns when the frame is complete (a host fb /
 * spp_out is copied back at the end).  A null scene, f, a or fb, a bad min_spp / max_spp, a non-finite threshold, a
 * non-finite or negative floor, or a bad frame size or partition is RT_ERR_INVALID before any HIP call, and
 * rt_last_error_detail() names the failed check.  The call is a frame of the scene: not re-entrant per scene; a pending
 * non-blocking rt_render of the scene is finished first.  Option "adaptive_tier": -1 (auto) = a pass runs on the tier
 * kernel when few pixels are active, 0 = always the main kernel, 1 = the tier kernel wherever the scene's tier data fit;
 * none changes a pixel. */
typedef struct rt_adaptive_desc {
    int32_t min_spp, max_spp;
    float threshold, floor;
} rt_adaptive_desc; /* 16 B */
rt_status rt_render_adaptive(rt_scene* scene, const rt_frame_desc* f, const rt_adaptive_desc* a, float* fb, int fb_on_device,
                             int32_t* spp_out, void* stream, rt_stats* stats);

/* ---- per-pixel variance: a frame plus an estimate of how noisy each of its pixels is ----
 * rt_render_variance renders the pixels the frame description assigns to the call (row partition as rt_render) at n = f->ns
 * samples and, beside the frame, writes per pixel the estimated variance of the pixel's mean of r + g + b, by batch means:
 * the n samples of a pixel are cut into B = v->batches consecutive batches of n / B samples, and the spread of the B batch
 * averages estimates the variance of their mean.  Parameters: 2 <= B <= 64 and n % B == 0 (so n >= B).
 * The contract, checkable from frames alone.  Let c_b = b * (n / B) for b = 0..B, and m_b the float triple the frame would
 * hold at ns = c_b with gamma 1 -- the colour sum of the first c_b samples times (float)(1.0 / (double)(float)c_b), per
 * channel, as store_pixel forms it (each pixel is one chain seeded by seed_base + its index, so the first c_b samples of a
 * frame at ns = n are the frame at ns = c_b); m_0 is not used.  Per pixel, in double, left to right, nothing contracted:
 *     s_b = ((double)m_b.x + (double)m_b.y) + (double)m_b.z,   T_b = (double)c_b * s_b,   T_0 = 0,
 *     y_b = (T_b - T_{b-1}) / (double)(n / B)                       for b = 1..B   (the average of batch b alone),
 *     A = A + y_b,   Q = Q + y_b * y_b,   both from 0,              for b = 1..B,
 *     mu = A / B,   v = Q / B - mu * mu,   v = (v > 0) ? v : 0      (so a NaN gives 0),
 *     variance_out = (float)(v / (double)(B - 1)).
 * fb is bit for bit what rt_render writes at ns = n with the frame's gamma; variance_out (required; the same kind of memory as
 * fb, compact local rows of nx floats) is linear whatever the gamma.  stats: rays and samples are rt_render's, ms_render = device
 * time from the first pass to the last, reserved = render passes (B).
 * Passes: [c_{b-1}, c_b) over every pixel, b = 1..B, each followed by one small kernel that updates 24 bytes per pixel; the
 * whole frame is enqueued on `stream` with no host round trip between passes, then the call waits for it (a host fb /
 * variance_out is copied back at the end).  The passes have no cost-aware schedule: a variance frame costs more than
 * rt_render's (measured 1.5 - 3.1 x).  A null scene, f, v, fb or variance_out, a B outside 2..64, an ns that is not a positive
 * multiple of B, or a bad frame size or partition is RT_ERR_INVALID before any HIP call, and rt_last_error_detail() names the
 * failed check.  The call is a frame of the scene: not re-entrant per scene; a pending non-blocking rt_render of the scene is
 * finished first. */
typedef struct rt_variance_desc { int32_t batches, reserved; } rt_variance_desc; /* 8 B */
rt_status rt_render_variance(rt_scene* scene, const rt_frame_desc* f, const rt_variance_desc* v, float* fb, int fb_on_device,
                             float* variance_out, void* stream, rt_stats* stats);

/* ---- denoiser, variance-guided: rt_denoise with a variance factor in the colour factor's place ----
 * rt_denoise's colour factor compares two noisy estimates with each other and so turns away exactly the noisy neighbours
 * that should be averaged.  rt_denoise_variance asks instead whether two pixels differ by more than their noise explains: it
 * takes the per-pixel variance rt_render_variance writes, filters it along with the colour, and weighs a tap by the squared
 * colour difference over the two pixels' variances.
 * Everything of rt_denoise's contract holds -- the arithmetic rule, the buffers, the workspace of rt_denoise_workspace_bytes
 * (it does not grow), option "denoise_lds", out == color -- with these differences:
 *   Parameters.  d->sigma_color must be 0 (the variance factor REPLACES the colour factor); vd->sigma_variance finite and in
 *     [1e-6, 1e6]; vd->variance_floor finite and > 0; vd->variance non-null: ny x nx floats, the variance of the mean of
 *     r + g + b per pixel.  vd->variance_out (ny x nx, optional) may overlap no other buffer.
 *   Prepare.  u = variance, or when demodulating, with a' = max(albedo, 2^-10) per channel at the same pixel:
 *     t = 3.0f / ((a'.r + a'.g) + a'.b),  u(q) = (variance(q) t) t.  v_0(p) is a 3x3 pre-blur of u: num = den = 0; for
 *     dy = -1..1 (outer), dx = -1..1 (inner), a tap outside the image is skipped, g = G[dy] G[dx] with G = {1/4, 1/2, 1/4},
 *     num = num + g u(q), den = den + g;  v_0 = num / den.
 *   Iteration k.  Every tap but the centre takes, after the normal and depth factors, one more factor on x_k and v_k:
 *     d1 = (|dr| + |dg|) + |db|;  den = (sigma_variance sigma_variance) (vp + vq) + variance_floor;  r = (d1 d1) / den;
 *     t = max(1 - r, 0);  the factor is t t.  Beside W and S every tap, the centre included, adds with its final w
 *     Sv = Sv + (w w) vq, Sv from 0;  after the 25 taps v_{k+1}(p) = Sv / (W W).
 *   Finish.  variance_out = (v_K / t) / t when demodulating (t of the pixel, as above), else v_K.
 * Only + - * /, max, abs and comparisons occur (max returns the other operand when one is a NaN); there is no square root.
 * The variance is expected to be finite and >= 0 (zeros are fine: the floor keeps den positive, a subnormal one included:
 * nothing is flushed to zero).  A negative or non-finite variance changes nothing beyond the pixels within reach of it --
 * 2 (2^K - 1) + 1 pixels each way, the pre-blur's one more; the same for an albedo when demodulating, 2 (2^K - 1) for the other
 * inputs -- and within reach the result is rt_denoise's rule: the restatement's, NaN for NaN.  Nothing faults: no address
 * depends on data.  tests/variance_expect.py restates this in NumPy float32; the device result equals it bit for bit.
 * A null d or vd and every violation above is RT_ERR_INVALID before any HIP call, and rt_last_error_detail() names the
 * failed check. */
typedef struct rt_denoise_variance_desc {
    const float* variance;     /* ny*nx, what rt_render_variance writes; required */
    float* variance_out;       /* ny*nx or null: the filtered variance */
    float sigma_variance, variance_floor;
} rt_denoise_variance_desc; /* 24 B */
rt_status rt_denoise_variance(const rt_denoise_desc* d, const rt_denoise_variance_desc* vd, int buffers_on_device, void* stream, int blocking);

/* ---- upscaler: joint bilateral upsampling of a coarse frame, guided by full-resolution feature buffers ----
 * u = (i + xi) / nx (main.cu:120-121), so a frame of nx/f x ny/f pixels on the same rt_camera is the same view, and coarse pixel
 * (I, J) covers the output pixels f I .. f I + f - 1 x f J .. f J + f - 1.  The paths cost 2-7 rays per sample at hundreds of
 * samples, the feature pass one primary ray per sample at 16 samples at most: rt_upscale rebuilds the nx x ny frame from paths
 * traced on the coarse grid and the guides of both grids.  It takes no scene and runs on the device the last rt_init selected.
 *
 * The numerical contract.  All arithmetic is binary32, every written operation is rounded once, nothing is contracted into
 * an FMA, sums run left to right as written; only + - * /, max, abs and comparisons occur (max returns the other operand when
 * one is a NaN); subnormal results are kept, never flushed to zero.  Images are whole frames, row-major,
 * row 0 at the bottom.  lx = nx / factor, ly = ny / factor.  color_lo (x3, required), albedo_lo (x3), normal_lo (x3) and
 * depth_lo (x1) are what rt_render (gamma 1) and rt_render_aov write for the lx x ly frame; albedo, normal and depth are what
 * rt_render_aov writes for the nx x ny frame of the same camera.
 *   Prepare.  demodulate != 0: x(Q) = color_lo(Q) / max(albedo_lo(Q), 2^-10) per channel (albedo_lo or albedo null is then
 *     RT_ERR_INVALID); otherwise x = color_lo.
 *   Position.  Output pixel p = (i, j), f = factor:  I = i / f (integers), r = i - I f;  J and s from j likewise.
 *     c = (float)(2 r + 1) / (float)(2 f) - 0.5f;  a = 0.5f - c;  b = 0.5f + c;
 *     B_x[-1] = 0.5f (a a);  B_x[0] = 0.75f - c c;  B_x[+1] = 0.5f (b b)  -- the quadratic B-spline: the three sum to one and
 *     reproduce a linear ramp.  B_y comes from s the same way.
 *   Taps.  W0 = W = 0, S0 = S = (0, 0, 0).  For dy = -1..1 (outer), dx = -1..1 (inner), Q = (I + dx, J + dy); a Q outside the
 *     coarse image is skipped.  g = B_y[dy] B_x[dx];  w = g, then w = w * factor for each factor that is on, in this order:
 *       normal  (normal and normal_lo non-null and normal_sharpness = m in 1..10; 0 = off):
 *               d = (Np.x Nq.x + Np.y Nq.y) + Np.z Nq.z;  d = max(d, 0);  then d = d d, m times;  the factor is d.
 *       depth   (depth and depth_lo non-null and sigma_depth > 0):
 *               den = sigma_depth max(Zp, Zq) + 1e-20f;  r = |Zp - Zq| / den;  t = max(1 - r, 0);  the factor is t t.
 *     Np, Zp are the output pixel's guides, Nq, Zq the coarse tap's.  Every tap takes the factors, the middle one included
 *     (there is no free centre tap as in rt_denoise: the middle tap is another pixel of another grid).  Then W0 = W0 + g,
 *     S0.ch = S0.ch + g x(Q).ch, W = W + w, S.ch = S.ch + w x(Q).ch.
 *   Choose.  guided = (W >= min_weight * W0) and (W > 0).  result.ch = S.ch / W when guided, else S0.ch / W0: the plain spline,
 *     for pixels no coarse tap resembles -- and for misses, whose normal is 0 and whose normal factor therefore is.  W0 > 0
 *     always: tap (I, J) is inside the coarse image and B[0] >= 0.5.
 *   Finish.  out = result * max(albedo(p), 2^-10) per channel when demodulating, else result.  No gamma is applied.
 *     weight_out = W / W0, whichever branch was taken.
 * tests/upscale_expect.py restates this in NumPy float32; the device result equals it bit for bit.  Inputs are expected to
 * be finite.  A NaN, an infinity or a negative depth or albedo in coarse pixel Q changes nothing beyond the output pixels with
 * I in Qx - 1 .. Qx + 1 and J in Qy - 1 .. Qy + 1, one in a full-resolution guide nothing beyond its own pixel; within that
 * reach out and weight_out are what the rules above give in IEEE 754 arithmetic with that max -- a NaN where the restatement
 * has one (sign and payload not specified), its bits elsewhere.  No value of any input makes the call fault: no address
 * depends on pixel data.  (tests/test_filter_domain.py)
 *
 * Parameters (anything else is RT_ERR_INVALID): factor 2..8; nx and ny positive multiples of it and nx ny < 2^31;
 * normal_sharpness 0..10; sigma_depth 0 or finite in [1e-6, 1e6]; min_weight finite and in [0, 1]; color_lo and out non-null;
 * normal and normal_lo both null or both given, depth and depth_lo likewise; out and weight_out share no byte with any other
 * buffer, where the host can see it (undefined otherwise).
 *
 * Buffers: rt_denoise's rules.  buffers_on_device != 0: every non-null buffer is device or managed memory of that device,
 * 4-byte aligned, checked with hipPointerGetAttributes before anything is launched; the work is enqueued on `stream` and
 * with `blocking` != 0 the call returns when out is written.  buffers_on_device == 0: host memory; the library stages the
 * buffers in device memory of the call's own, copies out and weight_out back and returns when it is complete, whatever
 * `blocking` says.  There is no workspace.  The argument checks run before any HIP call and rt_last_error_detail() names the
 * one that failed.  The call uses no scene and no shared state, so it may run beside a pending non-blocking rt_render on
 * another stream.  Option "upscale_lds": -1 (auto) and 1 = a workgroup prepares the coarse pixels its 16x16 output tile
 * reaches once, in LDS; 0 = every tap is read through L1/L2.  It changes no result. */
typedef struct rt_upscale_desc {
    int32_t nx, ny;            /* size of the output; lx = nx / factor, ly = ny / factor */
    int32_t factor;            /* 2..8; nx and ny must be multiples of it */
    int32_t normal_sharpness;  /* 0..10, 0 = normal factor off (rt_denoise's meaning) */
    int32_t demodulate, reserved;
    float sigma_depth;         /* 0 = off, else finite in [1e-6, 1e6] */
    float min_weight;          /* finite, in [0, 1] */
    const float* color_lo;     /* ly*lx*3, linear; required */
    const float* albedo_lo;    /* ly*lx*3 or null */
    const float* normal_lo;    /* ly*lx*3 or null */
    const float* depth_lo;     /* ly*lx   or null */
    const float* albedo;       /* ny*nx*3 or null */
    const float* normal;       /* ny*nx*3 or null */
    const float* depth;        /* ny*nx   or null */
    float* out;                /* ny*nx*3; required */
    float* weight_out;         /* ny*nx or null */
} rt_upscale_desc; /* 104 B */
rt_status rt_upscale(const rt_upscale_desc* d, int buffers_on_device, void* stream, int blocking);

/* ---- a camera per frame: another view of a scene that stays on the device ----
 * rt_scene_create copies the description's camera into the scene; rt_scene_set_camera replaces it, so that a turntable or a
 * viewport renders frame after frame without a second rt_scene_create (upload, tier data, calibration passes, regrouping and
 * collapse search).  Every kernel receives the camera by value at its launch, so the change costs the device nothing.
 *
 * Contract.  From the call on, every frame entry -- rt_render, rt_render_window, rt_render_adaptive, rt_render_variance,
 * rt_render_aov, rt_render_aov_through -- writes, bit for bit, what the same call writes on a scene made by rt_scene_create
 * from the same description with this camera in it, and reports the same rays and samples.  rt_trace_rays and
 * rt_radiance_rays do not read the camera.  The walk array, the tier data and the LDS plans are kept: any hierarchy over the
 * same leaves in the same order gives the reference's results for any ray; the one the scene walks was
 * chosen on the old camera's calibration frame and is merely no longer the measured optimum.
 * recalibrate == 0 keeps the cost prior of the old camera (the per-pixel ray counts of the calibration frame, which order
 * and split a ranked rt_render): it is then stale, which changes the schedule and never a pixel.  recalibrate != 0 renders
 * the calibration frame again -- 4 spp, its aspect taken from the new camera, its node pass counts thrown away -- and keeps
 * its costs: rt_debug_cal_cost returns the new grid.  A scene that kept no prior at creation gets none.
 * A pending non-blocking rt_render of the scene is finished first.  A progressive state made before the change keeps working
 * and its later windows use the new camera: what such a mixed accumulation means is the caller's business.
 * A null scene or camera, a non-finite field (pad is not looked at) or time1 < time0 is RT_ERR_INVALID before any HIP call,
 * and rt_last_error_detail() names the failed check.  rt_scene_get_camera returns the camera the next frame will use.
 * rt_multi_set_camera does the same for every replica of an rt_multi. */
rt_status rt_scene_set_camera(rt_scene* scene, const rt_camera* camera, int recalibrate);
rt_status rt_scene_get_camera(const rt_scene* scene, rt_camera* out);

/* ---- moving spheres: new sphere records for a scene that stays on the device ----
 * rt_scene_update_spheres replaces sphere records of a resident scene and refits every box that depends on them, on the device,
 * so that a simulation, a turntable with a moving light or an editor dragging a sphere renders step after step without a second
 * rt_scene_create (upload, three tree builds, four calibration passes, the collapse search).
 *
 * The update.  Record k of `spheres` replaces sphere indices[k], or sphere first + k when indices is null.  indices is host
 * memory always; spheres is host memory, or, with spheres_on_device != 0, device (or managed) memory of the scene's device (the
 * positions of a simulation that lives there; nothing is copied).  count == 0 is a successful no-op.
 *
 * Contract.  Let D' be the scene's description with those records replaced and its node boxes refit as below.  From the call on,
 * every frame entry -- rt_render, rt_render_window, rt_render_adaptive, rt_render_variance, rt_render_aov,
 * rt_render_aov_through -- and both query entries -- rt_trace_rays, rt_radiance_rays -- write, bit for bit, what they write on
 * rt_scene_create(D'), and report the same rays and samples.  The topology of every array on the device is kept: any hierarchy
 * over the same leaves in the same order gives the reference's results for any ray as long as every interior box contains the
 * boxes below it.
 *   Leaves that change.  A leaf is recomputed when its primitive is an updated sphere, or a constant_medium whose boundary is an
 *     updated sphere directly.  Every other leaf keeps its box, whatever rule made it.
 *   Box rule, as ordered binary32 operations, each rounded once, per axis:  r = |radius|,  a = c0 + 0 vel,  b = c0 + 1 vel,
 *     lo = min(a - r, b - r),  hi = max(a + r, b + r).  For radius >= 0 this is, value for value, the box the host library's
 *     sphere constructors give (the reference's sphere.cuh:21-38); for a negative radius it is a box that contains the shell.
 *   Refit.  Every interior node of the reference's tree and of the walk array becomes the float min / max union of the leaf boxes
 *     in its subtree; the tier data follow (leaf boxes and the per-64-leaf unions; padding leaves stay zero and take part in no
 *     union).  The scene's coordinate bound becomes, per axis, the maximum over all leaves of max(|bmin|, |bmax|) -- what
 *     rt_scene_create(D') computes; it may shrink.  The link words of a node (skip, prim) are never written.  Float min / max are
 *     exact, so boxes do not depend on the order of any reduction (up to the sign of a zero).
 *   What goes stale.  The walk array's choice of interior nodes and the cost prior were measured on the old positions; that
 *     changes time and never a pixel.  recalibrate != 0 redoes the cost half of the calibration exactly as rt_scene_set_camera
 *     does (the calibration frame at 4 spp, its per-pixel costs kept).
 * A pending non-blocking rt_render of the scene is finished first.  Progressive states behave as after a camera change: later
 * windows see the new spheres.  The work -- four small launches -- is enqueued on `stream` (a hipStream_t, 0 = default stream),
 * after whatever the stream already holds; other streams still reading the scene are the caller's to order.  The call is
 * SYNCHRONOUS: it returns after the work has completed, because it reads 16 bytes back (the new bound and the flag below).
 *
 * Refusals.  Each of these is RT_ERR_INVALID before any HIP call, with rt_last_error_detail() naming the check, and leaves the
 * scene untouched: a null scene, update or record array; count < 0; an index out of range; an index that appears twice; with
 * host records, a non-finite c0, vel or radius, or a mat outside the scene's materials; an updated sphere that is the child
 * of an instance -- reached as leaf -> instance or medium -> instance: its leaf's box follows the instance's rule, which a
 * sphere update does not redo.  Such a sphere still cannot change its own record; it moves with its instance instead
 * (rt_scene_update_instances, below), as direct spheres and sphere-bounded media move here.
 * Device-resident records cannot be checked on the host: the kernel that stores them checks each, stores nothing for a record
 * with a non-finite field or a bad mat and raises a flag that is read back with the bound; the call then returns RT_ERR_INVALID
 * with every record that passed applied and every box and union consistent with the spheres actually stored.  No address
 * depends on record data; the only data-derived addresses come from `indices`, which the host has checked.
 *
 * rt_scene_get_spheres copies the records the next frame will use to `out` (host memory, cap >= the scene's sphere count, else
 * RT_ERR_INVALID).  rt_multi_update_spheres applies host records to every replica of an rt_multi.
 * rt_refit_nodes is the host-only statement of D' (no device needed): nodes_out receives desc->n_nodes nodes -- the
 * description's with the leaves above recomputed and every interior box refit --, spheres_out desc->n_spheres records; either
 * may be null.  It makes rt_scene_create's checks of `desc` and the refusals above, and writes nothing when it refuses.
 * rt_debug_scene_boxes (tests): a device array of the scene as it stands, copied to host memory -- which = 0 the reference's
 * tree, 1 the walk array (both in the device's link encoding: skip holds ~skip, an interior prim ~(index + 1)), 2 / 3 the tier
 * leaf arrays, 4 the per-64-leaf unions (8 floats each), 5 the bound (3 floats).  *n = its bytes (0: the scene has none); at
 * most cap bytes are written. */
typedef struct rt_sphere_update {
    int32_t count;             /* records in `spheres` */
    int32_t first;             /* used when indices == NULL: record k replaces sphere first + k */
    const int32_t* indices;    /* or NULL; host memory always; each index at most once */
    const rt_sphere* spheres;  /* host memory, or device memory when spheres_on_device != 0 */
} rt_sphere_update; /* 24 B */
rt_status rt_scene_update_spheres(rt_scene* scene, const rt_sphere_update* update, int spheres_on_device, int recalibrate, void* stream);
rt_status rt_scene_get_spheres(const rt_scene* scene, rt_sphere* out, int32_t cap);
rt_status rt_refit_nodes(const rt_scene_desc* desc, const rt_sphere_update* update, rt_node* nodes_out, rt_sphere* spheres_out);   /* host only, no device */
rt_status rt_debug_scene_boxes(const rt_scene* scene, int32_t which, void* out, size_t cap, size_t* n);

/* ---- moving instances: new instance records for a scene that stays on the device ----
 * rt_scene_update_instances replaces instance records -- translate(rotate_y(child)) -- of a resident scene and refits every box
 * that depends on them, on the device: the blocks of a Cornell box turn, a fog volume bounded by an instance drifts, a crowd of
 * rotated boxes moves at once, frame after frame without a second rt_scene_create.
 *
 * The update.  Record k of `instances` replaces instance indices[k], or instance first + k when indices is null.  indices is
 * host memory always; instances is host memory, or, with instances_on_device != 0, device (or managed) memory of the scene's
 * device (nothing is copied).  count == 0 is a successful no-op.
 *
 * Contract.  Let D' be the scene's description with those records replaced and its node boxes refit as below.  From the call on,
 * every frame entry -- rt_render, rt_render_window, rt_render_adaptive, rt_render_variance, rt_render_aov,
 * rt_render_aov_through -- and both query entries -- rt_trace_rays, rt_radiance_rays -- write, bit for bit, what they write on
 * rt_scene_create(D'), and report the same rays and samples.  Topology, link words, the walk array's choice of nodes and the
 * tier arrays' .w words are never written.
 *   What a record may change.  sin_t, cos_t, offset and flags.  flags must be 1, 2 or 3 (RT_INST_ROTATE_Y, RT_INST_TRANSLATE or
 *     both): rt_scene_create's kernels and the oracle know nothing else.  child must equal the child the scene holds for that
 *     instance: the tier arrays and the per-kind passes were built on it.  pad is not looked at (and stored as given).
 *   Leaves that change.  A leaf is recomputed when its primitive is an updated instance, or a constant_medium whose boundary is
 *     an updated instance directly.  Every other leaf keeps its box, whatever rule made it (a generated description may carry
 *     outward-rounded boxes; an instance's leaf keeps such a box until that instance is updated).
 *   Box rule, as ordered binary32 operations, each rounded once, nothing contracted except the two fmaf written here.
 *     1. The child's box (lo, hi) in object space.  Sphere: the sphere rule above.  Quad:  p = (Q + u) + v,
 *        lo = min(min(Q, p), min(Q + u, Q + v)) - 1e-3f,  hi = max(max(Q, p), max(Q + u, Q + v)) + 1e-3f  per axis.  Box: the
 *        min / max of the quad rule over its six quads first_quad .. first_quad + 5, in that order.
 *     2. flags & RT_INST_ROTATE_Y:  from lo' = FLT_MAX, hi' = -FLT_MAX, the eight corners (x, y, z) of the child's box in the
 *        order i, j, k = 0..1 (x outer, z inner; 0 takes lo, 1 takes hi):  rx = fmaf(cos_t, x, sin_t * z),  ry = y,
 *        rz = fmaf(cos_t, z, -(sin_t * x)),  then lo' = min(lo', r), hi' = max(hi', r).
 *     3. flags & RT_INST_TRANSLATE:  lo + offset,  hi + offset.
 *     This is, value for value, what the host library's constructors give (quad::quad, compound6, rotate_y::rotate_y and
 *     translate in host/rtw.cpp and rtw.h; the reference's quad.cuh:29-54, 108-122 and hittable.cuh:40-116), so that writing a
 *     flattened scene's own records back changes no box; tests/test_update_instances_host.py pins that on five named scenes.
 *     With a (sin_t, cos_t) that is no sine / cosine pair the box need not contain the object -- which is what
 *     rt_scene_create of such a description gives too, so the contract holds all the same.
 *   Refit.  As after a sphere update: interior boxes of both node arrays, the tier leaf boxes and per-64-leaf unions, the bound.
 *   What goes stale.  The cost prior and the cost map, exactly as after a sphere update; recalibrate != 0 redoes the cost half
 *     of the calibration and drops the map.
 * A pending non-blocking rt_render of the scene is finished first.  The work -- four small launches -- is enqueued on `stream`
 * after whatever it holds.  The call is SYNCHRONOUS: it reads 16 bytes back (the new bound and the flag below).
 *
 * Refusals.  Each of these is RT_ERR_INVALID before any HIP call, with rt_last_error_detail() naming the check after
 * "rt_scene_update_instances: " (or "rt_refit_instances: "), and leaves the scene untouched: a null scene, update or record
 * array; count < 0; an index out of range; an index that appears twice; with host records, a non-finite sin_t, cos_t or offset,
 * flags outside 1..3, or a child other than the scene's.
 * Device-resident records are checked by the kernel that stores them: a record with a non-finite field, bad flags or another
 * child is not stored, a flag is read back with the bound, and the call returns RT_ERR_INVALID with every record that passed
 * applied and every box consistent with the records actually stored.  No address depends on record data: the child a box is
 * computed from is the scene's own, validated at creation, never the incoming record's; the only data-derived addresses come
 * from `indices`, which the host has checked.
 *
 * What still cannot move: a sphere record under an instance (rt_scene_update_spheres refuses it; the sphere moves with its
 * instance), and an instance's child.  Quads and boxes, under an instance or not, change through rt_scene_update_quads (below).
 * rt_scene_get_instances copies the records the next frame will use (cap >= the scene's instance count, else RT_ERR_INVALID).
 * rt_multi_update_instances applies host records to every replica of an rt_multi.  rt_refit_instances is the host-only statement
 * of D' (no device needed), as rt_refit_nodes: nodes_out receives desc->n_nodes nodes, instances_out desc->n_instances records;
 * either may be null; it makes rt_scene_create's checks of `desc` and the refusals above and writes nothing when it refuses. */
typedef struct rt_instance_update {
    int32_t count;                 /* records in `instances` */
    int32_t first;                 /* used when indices == NULL: record k replaces instance first + k */
    const int32_t* indices;        /* or NULL; host memory always; each index at most once */
    const rt_instance* instances;  /* host memory, or device memory when instances_on_device != 0 */
} rt_instance_update; /* 24 B */
rt_status rt_scene_update_instances(rt_scene* scene, const rt_instance_update* update, int instances_on_device, int recalibrate, void* stream);
rt_status rt_scene_get_instances(const rt_scene* scene, rt_instance* out, int32_t cap);
rt_status rt_refit_instances(const rt_scene_desc* desc, const rt_instance_update* update, rt_node* nodes_out, rt_instance* instances_out);   /* host only, no device */

/* ---- moving quads and boxes: new quad records for a scene that stays on the device ----
 * rt_scene_update_quads replaces quad records of a resident scene -- free quads, the six faces of a box, either of them under an
 * instance or around a constant_medium -- and refits every box that depends on them, on the device: the light and the walls of a
 * Cornell box, a door, a ground plate, a lid that opens, a box that changes size, frame after frame without a second
 * rt_scene_create.
 *
 * The update.  Record k of `quads` replaces quad indices[k], or quad first + k when indices is null.  indices is host memory
 * always; quads is host memory, or, with quads_on_device != 0, device (or managed) memory of the scene's device (nothing is
 * copied).  count == 0 is a successful no-op.  A box changes through its faces: quads first_quad .. first_quad + 5.
 *
 * Contract.  Let D' be the scene's description with those records replaced and its node boxes refit as below.  From the call on,
 * every frame entry -- rt_render, rt_render_window, rt_render_adaptive, rt_render_variance, rt_render_aov,
 * rt_render_aov_through -- and both query entries -- rt_trace_rays, rt_radiance_rays -- write, bit for bit, what they write on
 * rt_scene_create(D'), and report the same rays and samples.  Topology, link words, the walk array's choice of nodes and the
 * tier arrays' .w words are never written.
 *   What a record may change.  Every geometric field (Q, D, u, v, w, n) and mat.  The caller supplies the derived fields D, w
 *     and n as a description does (n the unit normal, D = n . Q, w = (u x v) / |u x v|^2); their consistency with Q, u, v is not
 *     checked, exactly as rt_scene_create does not check it.  pad0 is not looked at; pad1 and pad2 are stored as given.
 *   Derived device data.  rt_scene_create keeps two things it derives from quad records: the axis code of every quad (in the
 *     device copy's pad0: 1 + C for a quad whose unit normal is exactly +-e_C and whose u, v, w each have exactly one non-zero
 *     component on the fitting axes, else 0) and the canonical mark of every box (bit 30 of the device copy's first_quad: its six
 *     faces carry the codes 3, 1, 3, 1, 2, 2 -- normals along z, x, z, x, y, y -- in order).  They select the axis-aligned quad
 *     test and the six-face fast path.  The update stores the axis code of every incoming record by the same function creation
 *     uses, and, after all records are stored, recomputes the mark of every box from its six faces (box ranges may overlap, so
 *     the decision is per box, in a launch of its own after the one that stores).  rt_scene_get_quads returns pad0 as +0.0f.
 *   Leaves that change.  Call a leaf's solid its primitive, or, for a constant_medium, that medium's boundary.  A leaf is
 *     recomputed when its solid is an updated quad, a box with at least one updated face, or an instance whose child is either
 *     of those (one box under several instances recomputes every one of those leaves).  Every other leaf keeps its box, whatever
 *     rule made it (a generated description may carry outward-rounded boxes; such a leaf keeps its box until something under it
 *     is updated).
 *   Box rule.  The quad rule, the box rule and the instance rule over the child's box, as stated for rt_scene_update_instances
 *     above: value for value what the host library's constructors give (quad::quad, compound6, rotate_y, translate), so that
 *     writing a flattened scene's own records back changes no box; tests/test_update_quads_host.py pins that on named scenes.
 *   Refit, what goes stale, recalibrate, a pending frame, progressive states, the cost map: as after a sphere update.
 * The work -- five small launches -- is enqueued on `stream` after whatever it holds.  The call is SYNCHRONOUS: it reads 16 bytes
 * back (the new bound and the flag below).
 *
 * Refusals.  Each of these is RT_ERR_INVALID before any HIP call, with rt_last_error_detail() naming the check after
 * "rt_scene_update_quads: " (or "rt_refit_quads: "), and leaves the scene untouched: a null scene, update or record array;
 * count < 0; an index out of range; an index that appears twice; with host records, a non-finite Q, D, u, v, w or n, or a mat
 * outside the scene's materials.  A quad under an instance is allowed.
 * Device-resident records are checked by the kernel that stores them: a record with a non-finite field or a bad mat is neither
 * stored nor stamped, a flag is read back with the bound, and the call returns RT_ERR_INVALID with every other record applied
 * and every box and mark consistent with the records actually stored.
 * Memory safety.  No address depends on record data.  Addresses come only from the index list, which the host has checked; from a
 * per-leaf table the host makes from the scene's own leaves (the solid each leaf follows); from the scene's stored instance
 * child; and from boxes[..].first_quad with its mark bits masked -- all validated by rt_scene_create and never written from an
 * incoming record (the update writes bit 30 of first_quad only).
 *
 * What it does not do: rt_reproject, rt_reproject_moving and rt_reproject_instances do not follow a moved quad; their tap tests
 * reject such pixels, which then restart their history.  rt_reproject_quads, below, follows it.
 * rt_scene_get_quads copies the records the next frame will use, pad0 zeroed (cap >= the scene's quad count, else
 * RT_ERR_INVALID).  rt_multi_update_quads applies host records to every replica of an rt_multi.  rt_refit_quads is the host-only
 * statement of D' (no device needed), as rt_refit_nodes: nodes_out receives desc->n_nodes nodes, quads_out desc->n_quads records
 * (the incoming records as given, pad0 included); either may be null; it makes rt_scene_create's checks of `desc` and the
 * refusals above and writes nothing when it refuses.
 * rt_debug_scene_quads (tests): the device's quad and box records raw, marks included -- pad0 holds the axis code as an integer,
 * first_quad bit 30 the canonical mark; quad_cap / box_cap >= the scene's counts, else RT_ERR_INVALID; either output may be null. */
typedef struct rt_quad_update {
    int32_t count;            /* records in `quads` */
    int32_t first;            /* used when indices == NULL: record k replaces quad first + k */
    const int32_t* indices;   /* or NULL; host memory always; each index at most once */
    const rt_quad* quads;     /* host memory, or device memory when quads_on_device != 0 */
} rt_quad_update; /* 24 B */
rt_status rt_scene_update_quads(rt_scene* scene, const rt_quad_update* update, int quads_on_device, int recalibrate, void* stream);
rt_status rt_scene_get_quads(const rt_scene* scene, rt_quad* out, int32_t cap);
rt_status rt_refit_quads(const rt_scene_desc* desc, const rt_quad_update* update, rt_node* nodes_out, rt_quad* quads_out);   /* host only, no device */
rt_status rt_debug_scene_quads(const rt_scene* scene, rt_quad* quads_out, int32_t quad_cap, rt_box* boxes_out, int32_t box_cap);

/* ---- temporal reprojection: the current frame blended into the reprojected history of the previous one ----
 * With a camera that moves, the samples of one frame can be reused in the next: rt_reproject finds, for every pixel of the
 * current frame, where its surface point was in the previous frame (through the depth rt_render_aov writes and the two
 * cameras), fetches the accumulated history there -- four taps, each checked against the previous frame's feature buffers --
 * and blends the current frame in with weight 1 / (history length + 1).  Its outputs are the next call's history.  It takes no
 * scene and runs on the device the last rt_init selected.
 *
 * The numerical contract.  All arithmetic is binary32 unless stated, every written operation is rounded once, nothing is
 * contracted into an FMA, sums run left to right as written; only + - * /, floor, min, max, abs and comparisons occur
 * (min and max return the other operand when one is a NaN).  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.  Images are whole
 * unpartitioned frames of ny x nx pixels, row-major, row 0 at the bottom.
 *   Matrix (rt_reproject_matrix; host, in double from the float fields of `prev`, uncontracted).  A = LL - O (lower_left_corner
 *     - origin), H = horizontal, V = vertical;  cross(x, y) = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0);  r0 = H x V,
 *     r1 = V x A, r2 = A x H;  D = (A0 r0_0 + A1 r0_1) + A2 r0_2;  M[k][c] = (float)(r_k[c] / D), m[3 k + c].  So for
 *     q = a (A + s H + t V):  dot(M0, q) = a, dot(M1, q) = a s, dot(M2, q) = a t.  D == 0 or a non-finite M is RT_ERR_INVALID.
 *     rt_reproject calls it for d->prev.
 *   Pixel p = (i, j).
 *   1. s = ((float)i + 0.5f) / (float)nx, t = ((float)j + 0.5f) / (float)ny;  dir.c = ((LL.c + s H.c) + t V.c) - O.c of `cur`,
 *      per component (the centre ray: no lens offset).  surface = alpha[p] >= alpha_min.  Surface: z = depth[p] / alpha[p],
 *      P.c = O.c + z dir.c, q.c = P.c - O'.c, O' the origin of `prev`.  Otherwise the pixel is sky, a point at infinity: q = dir.
 *   2. a = dot(M0, q), b = dot(M1, q), c = dot(M2, q).  Unless a > 0 the pixel has no history.  x = (b / a) (float)nx - 0.5f,
 *      y = (c / a) (float)ny - 0.5f;  x0 = floor(x), y0 = floor(y), fx = x - x0, fy = y - y0.  Unless x0 >= -1, x0 <= (float)(nx - 1),
 *      y0 >= -1 and y0 <= (float)(ny - 1) the pixel has no history: float comparisons made before any conversion, so a NaN
 *      ends here.
 *   3. The taps q_k = (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), in this order, with the weights
 *      (1 - fx) (1 - fy), fx (1 - fy), (1 - fx) fy, fx fy.  A tap counts iff it is inside the image, history_len[q] > 0, it
 *      passes the geometry test -- surface pixel: prev_alpha[q] >= alpha_min and, with zq = prev_depth[q] / prev_alpha[q],
 *      |zq - a| <= depth_tol max(zq, a);  sky pixel: prev_alpha[q] < alpha_min -- and, with normals on and on a surface pixel,
 *      dot(normal[p], prev_normal[q]) >= normal_min, and, with ids on, prim[p] == prev_prim[q].  Each counting tap does
 *      W = W + w, C.ch = C.ch + w history[q].ch, L = L + w history_len[q], all from 0.
 *   4. W > 0: h = C / W per channel, n = min(L / W, max_history), out_len = n + 1, g = 1 / out_len,
 *      out.ch = h.ch + (color.ch - h.ch) g.  No history, or a null `history` (the first frame): out = color, out_len = 1.
 *      motion = (x - (float)i, y - (float)j) whenever step 2 produced x and y (a > 0), else (0, 0); it does not need a history.
 * tests/reproject_expect.py restates this in NumPy; the device result equals it bit for bit.
 * Limits.  The centre ray ignores the lens and the shutter: under defocus, or with spheres that have a velocity, the
 * reprojection is approximate (the geometry test then rejects more).  rt_reproject assumes that the world stood still between
 * the two frames: a sphere whose record changed (rt_scene_update_spheres) is rejected by the tap tests, not followed --
 * rt_reproject_moving, below, follows it.  depth and alpha must be rt_render_aov's; rt_render_aov_through's depth
 * runs along a bent path and is not geometric.  Normals are on iff normal and prev_normal are both non-null, ids iff prim and
 * prev_prim are.
 * Memory safety.  No address depends on a value that has not passed the comparisons of steps 2 and 3; no value of any input
 * makes the call fault.
 *
 * Parameters (anything else is RT_ERR_INVALID): nx, ny >= 1 and nx ny < 2^31; alpha_min in (0, 1]; depth_tol finite in [0, 1];
 * normal_min finite in [-1, 1]; max_history finite in [1, 65536]; color, depth, alpha, out and out_len non-null; history_len,
 * prev_depth and prev_alpha non-null iff history is; no output may overlap an input or another output where the host can see
 * it.  Buffers, stream and blocking: rt_denoise's rules -- buffers_on_device != 0: device or managed memory of that device,
 * 4-byte aligned, checked with hipPointerGetAttributes before anything is launched, the work enqueued on `stream` and waited
 * for only with `blocking` != 0; buffers_on_device == 0: host memory staged in device memory of the call's own, and the call
 * returns when the outputs are complete.  The argument checks run before any HIP call and rt_last_error_detail() names the one
 * that failed.  No scene and no shared state: the call may run beside a pending non-blocking rt_render on another stream. */
typedef struct rt_reproject_desc {
    int32_t nx, ny;
    rt_camera cur, prev;            /* cameras of the current and the previous frame */
    const float* color;             /* ny*nx*3 current linear frame, required */
    const float* depth, *alpha;     /* current rt_render_aov depth and alpha, required */
    const float* normal;            /* current, ny*nx*3 or null */
    const int32_t* prim;            /* current, or null */
    const float* history;           /* ny*nx*3 previous OUTPUT of this call; null = first frame */
    const float* history_len;       /* ny*nx previous out_len; required iff history */
    const float* prev_depth, *prev_alpha;   /* required iff history */
    const float* prev_normal;       /* used iff normal and prev_normal both non-null */
    const int32_t* prev_prim;       /* used iff prim and prev_prim both non-null */
    float* out;                     /* ny*nx*3 required */
    float* out_len;                 /* ny*nx required */
    float* motion;                  /* ny*nx*2 or null: (x - i, y - j), 0 where nothing was projected */
    float alpha_min, depth_tol, normal_min, max_history;
} rt_reproject_desc;
rt_status rt_reproject(const rt_reproject_desc* d, int buffers_on_device, void* stream, int blocking);
rt_status rt_reproject_matrix(const rt_camera* prev, float m[9]);   /* host only, no device */

/* ---- temporal reprojection that follows moved spheres ----
 * rt_reproject_moving is rt_reproject with one more step: a surface pixel whose first-hit primitive is a sphere whose record
 * changed between the two frames (rt_scene_update_spheres) -- or a constant_medium bounded directly by such a sphere -- is
 * carried back to where that surface point was in the previous frame, and only then projected into the previous camera.  A
 * sphere that translates and changes its radius maps its surface onto itself by a similarity (P - c) r' / r + c', which is
 * exact for the sphere's own surface and an approximation for a scattering point inside a fog ball.
 *
 * The numerical contract extends rt_reproject's and keeps its rules: binary32, every written operation rounded once, nothing
 * contracted, the operand order as written.  Ids are required: d->prim and d->prev_prim must be non-null (without them nothing
 * says which sphere a pixel shows, and nothing rejects the background a sphere uncovered); the id test of a tap is always on.
 * Steps 2-4 are rt_reproject's.  Step 1 gains a tail for surface pixels only (sky never follows):
 *   1a. Which sphere.  ref = prim[p], k = none.  ref >= 0 and ref >> 28 == RT_PRIM_SPHERE: k = ref & 0x0FFFFFFF.  ref >= 0,
 *       ref >> 28 == RT_PRIM_MEDIUM and (ref & 0x0FFFFFFF) < n_media: b = media[ref & 0x0FFFFFFF].boundary, and if b >= 0 and
 *       b >> 28 == RT_PRIM_SPHERE then k = b & 0x0FFFFFFF.  Unless k < n_spheres (compared unsigned, before any address is
 *       formed) the pixel is static.
 *   1b. The two centres.  S = spheres[k], S' = prev_spheres[k];  cc.c = S.c0.c + time S.vel.c,  cp.c = S'.c0.c + prev_time S'.vel.c
 *       per component;  moved = cc.x != cp.x || cc.y != cp.y || cc.z != cp.z || S.radius != S'.radius (a NaN compares as moved).
 *       Unless moved the pixel is static: its q is rt_reproject's, bit for bit.
 *   1c. The carry.  ratio = S'.radius / S.radius;  P'.c = cp.c + (P.c - cc.c) ratio;  q.c = P'.c - O'.c.  A zero or non-finite
 *       radius yields a non-finite q, which the a > 0 test and the float comparisons of step 2 end with no history.
 * motion is written as before from the x, y of step 2: for a followed pixel it is the object's motion plus the camera's.
 * So with n_spheres == 0, or with tables in which no record moved, the outputs are rt_reproject's bit for bit; and a sphere
 * under an instance, which cannot be updated, never differs: its pixel (prim = the sphere, inst >= 0) takes the static path
 * and no inst buffer is needed.  tests/reproject_moving_expect.py restates this in NumPy; the device result equals it bit for bit.
 * Limits.  As before the centre ray ignores the lens and the shutter; a sphere with vel != 0 is followed at one instant per
 * frame (`time`, `prev_time`; the binding's default is each camera's shutter centre, (float)(0.5 (time0 + time1))).  A quad or
 * box that is not under an instance and a sphere record under an instance do not move in this project; an instance does
 * (rt_scene_update_instances), but its motion is not followed by this entry: a pixel on a moved instance takes the static path, and the
 * taps' depth, normal and id tests decide whether its history survives -- rt_reproject_instances, below, follows it.  Reflections
 * of a moved sphere in other surfaces are not followed.
 * Memory safety.  Two kinds of data-derived addresses are added: media[...] after the unsigned compare against n_media, and
 * spheres[k] / prev_spheres[k] after the unsigned compare against n_spheres.  Nothing loaded from a record reaches an address;
 * no value in any buffer or table makes the call fault.
 *
 * Parameters: everything rt_reproject refuses, and a null m, a null prim or prev_prim, a negative count, n_spheres > 0 with a
 * null spheres or prev_spheres, n_media > 0 with a null media, a count of 2^28 or more, a non-finite time or prev_time and an
 * output that overlaps one of the tables are RT_ERR_INVALID before any HIP call; rt_last_error_detail() names the check and
 * starts with "rt_reproject_moving".  The tables obey buffers_on_device like every other buffer (device or managed memory of
 * the device, checked with hipPointerGetAttributes; host memory is staged); a table whose count is 0 is not looked at.  Stream
 * and blocking: rt_reproject's rules. */
typedef struct rt_reproject_motion_desc {
    int32_t n_spheres, n_media;       /* lengths of the tables; 0 with null tables is allowed */
    const rt_sphere* spheres;         /* the records the CURRENT frame was rendered with */
    const rt_sphere* prev_spheres;    /* the records the PREVIOUS frame was rendered with, same count and order */
    const rt_medium* media;           /* the scene's media (their boundaries say which sphere a fog ball follows), or null */
    float time, prev_time;            /* the instants at which centres are evaluated: c = c0 + time * vel */
} rt_reproject_motion_desc;
rt_status rt_reproject_moving(const rt_reproject_desc* d, const rt_reproject_motion_desc* m,
                              int buffers_on_device, void* stream, int blocking);

/* ---- temporal reprojection that follows moved instances ----
 * rt_reproject_instances is rt_reproject_moving with one more rule: a surface pixel that shows an instance whose record changed
 * between the two frames (rt_scene_update_instances) -- or a constant_medium bounded directly by such an instance -- is carried
 * back to where that surface point was in the previous frame: into the instance's object space by the current record, out of it
 * by the previous one.  An instance rotates, so the pixel's normal is carried the same way before the normal test; and one child
 * can sit under several instances, so the primitive id alone does not say which object a pixel shows: the entry takes the two
 * `inst` planes of rt_render_aov and a tap must show the pixel's instance.
 *
 * m is required: it supplies the media table, the two times and the sphere tables, and may have n_spheres = 0.  The numerical
 * contract is rt_reproject_moving's (binary32, every written operation rounded once, nothing contracted -- the walk that renders
 * an instance uses fmaf for the same maps, this entry does not) with these changes to step 1's tail (surface pixels only) and
 * to step 3:
 *   1a'. Which instance.  i = none.  inst[p] >= 0: i = inst[p].  Otherwise, if ref = prim[p] has ref >= 0, ref >> 28 ==
 *        RT_PRIM_MEDIUM and (ref & 0x0FFFFFFF) < n_media (unsigned): b = media[ref & 0x0FFFFFFF].boundary, and if b >= 0 and
 *        b >> 28 == RT_PRIM_INSTANCE then i = b & 0x0FFFFFFF.  If i < n_instances (compared unsigned, before any address is
 *        formed) the pixel takes the instance path and steps 1a-1c are skipped: a sphere under an instance holds object-space
 *        records, for which a world-space sphere carry would be wrong.  Otherwise steps 1a-1c of rt_reproject_moving apply
 *        unchanged.
 *   1b'. Moved.  I = instances[i], I' = prev_instances[i].  moved = any of sin_t, cos_t, offset[0..2] compares != or the flags
 *        differ (a NaN compares as moved; child and pad are not looked at).  Unless moved the pixel is static: its q and its
 *        normal are rt_reproject's, bit for bit.
 *   1c'. The carry.  A = P;  I.flags & RT_INST_TRANSLATE: A.c = P.c - I.offset.c.
 *        B = A;  I.flags & RT_INST_ROTATE_Y: B.x = I.cos_t A.x - I.sin_t A.z,  B.z = I.sin_t A.x + I.cos_t A.z  (world -> object).
 *        C = B;  I'.flags & RT_INST_ROTATE_Y: C.x = I'.cos_t B.x + I'.sin_t B.z,  C.z = I'.cos_t B.z - I'.sin_t B.x  (object ->
 *        previous world).  P' = C;  I'.flags & RT_INST_TRANSLATE: P'.c = C.c + I'.offset.c.  q.c = P'.c - O'.c.
 *        With normals on, N = normal[p] goes through the same two rotations (B and C with N in A's place, no translation), and
 *        step 3's normal test reads dot(N_carried, prev_normal[q]) >= normal_min.  Flag bits are only tested: flags outside
 *        1..3 reach no address.  A non-finite record yields a non-finite q, which step 2 ends with no history.
 *   3.   A tap must also satisfy inst[p] == prev_inst[q].  This test is always on, as the prim test is in rt_reproject_moving:
 *        it is what tells two instances of one child apart.
 * So with n_instances == 0, or with tables in which no record differs and inst equal to -1 everywhere, the outputs are
 * rt_reproject_moving's bit for bit, and by that entry's own identity rt_reproject's.  tests/reproject_instances_expect.py
 * restates this in NumPy; the device result equals it bit for bit.
 * Limits.  The carry is exact for a rigid surface and an approximation for a scattering point in a fog volume bounded by an
 * instance, as the sphere carry is for a fog ball.  A quad's normal is oriented to face the ray, and that orientation can flip
 * between two frames: the normal test then rejects the tap.  Reflections of a moved instance in other surfaces are not followed.
 * The centre ray ignores the lens and the shutter, as before.
 * Memory safety.  The data-derived addresses that are added are instances[i] and prev_instances[i] after the unsigned compare
 * against n_instances, and inst[...] / prev_inst[...] at the pixel and tap indices that rt_reproject's rules already bound.
 * Nothing loaded from a record reaches an address; no value in any buffer or table makes the call fault.
 *
 * Parameters: everything rt_reproject_moving refuses, and a null im, a null inst, a prev_inst that is null while history is not
 * (or the reverse), a negative n_instances or one of 2^28 or more, n_instances > 0 with a null instances or prev_instances, and
 * an output that overlaps one of the new tables or planes are RT_ERR_INVALID before any HIP call; rt_last_error_detail() names
 * the check and starts with "rt_reproject_instances".  The tables and planes obey buffers_on_device like every other buffer; a
 * table whose count is 0 is not looked at.  Stream and blocking: rt_reproject's rules. */
typedef struct rt_reproject_instance_desc {
    int32_t n_instances, reserved;
    const rt_instance* instances;        /* records the CURRENT frame was rendered with */
    const rt_instance* prev_instances;   /* records the PREVIOUS frame was rendered with, same count and order */
    const int32_t* inst;                 /* ny*nx current rt_render_aov `inst`, required */
    const int32_t* prev_inst;            /* ny*nx previous; required iff d->history */
} rt_reproject_instance_desc;
rt_status rt_reproject_instances(const rt_reproject_desc* d, const rt_reproject_motion_desc* m,
                                 const rt_reproject_instance_desc* im, int buffers_on_device, void* stream, int blocking);

/* ---- temporal reprojection that follows moved quads and boxes ----
 * rt_reproject_quads is rt_reproject_instances with one more rule: a surface pixel that shows a quad whose record changed between
 * the two frames (rt_scene_update_quads) -- a free quad or a face of a box, in world space or under an instance -- is carried back
 * to where that point of the quad was in the previous frame.  A quad maps onto its previous self by an affine map of its own
 * plane: the point keeps its planar coordinates (alpha, beta), those of quad::hit, and is rebuilt from the previous record's Q, u
 * and v.  A quad under an instance holds object-space records, so the carry happens between the two instance maps of
 * rt_reproject_instances, whether or not the instance itself moved.  The stored normal changes with the record: the carried
 * normal is the previous record's n, on the side of the quad the pixel saw.  A box follows face by face: prim names the face.
 *
 * m and im are required: m may hold no sphere and im no instance record, but im->inst stays required -- it says in whose object
 * space a quad's record lives.  The numerical contract is rt_reproject_instances' (binary32, every written operation rounded
 * once, nothing contracted, operands in the order written, only + - * / and comparisons; dot and cross as defined above) with
 * this rule in front of step 1's tail (surface pixels only):
 *   1a''. Which quad.  ref = prim[p].  If ref >= 0 and ref >> 28 == RT_PRIM_QUAD: g = ref & 0x0FFFFFFF.  The pixel takes the quad
 *        path iff g < n_quads (compared unsigned, before any address is formed) and inst[p] < 0 or inst[p] < n_instances
 *        (unsigned).  An inst[p] >= n_instances means object-space records of an instance the tables do not describe: such a
 *        pixel does not take the quad path.  Every other pixel follows rt_reproject_instances' step 1 unchanged -- a pixel
 *        whose prim is a medium included: a fog volume bounded by a quad, a box or an instance of one does not say which face
 *        a scattering point belongs to.
 *   1b''. Moved.  G = quads[g], G' = prev_quads[g].  qmoved = any component of Q, u or v compares != (a NaN compares as moved;
 *        D, w, n, mat and the pads do not enter).  With an instance i = inst[p] in range, imoved is the `moved` of 1b'.  Neither: the
 *        pixel's q and normal are rt_reproject's, bit for bit.  imoved only: step 1c', bit for bit.
 *   1c''. The carry, when qmoved.  B is the object-space point: with i in range, A and B of 1c' by the current record I (applied
 *        whether or not the instance moved); otherwise B = P.
 *        h.c = B.c - G.Q.c;  x = cross(h, G.v);  y = cross(G.u, h);  alpha = dot(G.w, x);  beta = dot(G.w, y)  (not clamped).
 *        B'.c = (G'.Q.c + alpha G'.u.c) + beta G'.v.c.
 *        With i in range P' comes from B' by the previous record I' (C and P' of 1c' with B' in B's place); otherwise P' = B'.
 *        q.c = P'.c - O'.c.
 *        With normals on: Nb = normal[p] through I's rotation (B of 1c' with N in A's place; normal[p] itself with no instance),
 *        s = dot(Nb, G.n), Nb'.c = s G'.n.c -- the side of the quad the pixel saw and its sample-averaged length -- and Nb'
 *        goes through the previous record's rotation (C of 1c') before step 3 tests it.
 *        A non-finite record yields a non-finite q, which step 2 ends with no history.  A zero w yields P' = G'.Q: finite,
 *        wrong and harmless.
 *   3.   rt_reproject_instances': the prim and inst tests are always on, so a tap must show the same quad of the same instance.
 * So with n_quads == 0, or with tables in which no record differs in Q, u or v, the outputs are rt_reproject_instances' bit for
 * bit, and by that entry's identities rt_reproject_moving's and rt_reproject's.  tests/reproject_quads_expect.py restates this in
 * NumPy; the device result equals it bit for bit.
 * Limits.  Media are not followed by this rule.  A quad's normal is oriented to face the ray, and that orientation can flip
 * between two frames: the normal test then rejects the tap.  Reflections of a moved quad in other surfaces are not followed.
 * The centre ray ignores the lens and the shutter, as before.  The carry is exact for points of the quad's plane; for a depth
 * that is a mean over samples it is the projection along n.
 * Memory safety.  The only data-derived addresses that are added are quads[g] and prev_quads[g], formed after the unsigned
 * compare against n_quads.  Nothing loaded from a record reaches an address; no value in any buffer or table makes the call
 * fault.
 *
 * Parameters: everything rt_reproject_instances refuses, and a null qm, a negative n_quads or one of 2^28 or more, n_quads > 0
 * with a null quads or prev_quads, and an output that overlaps one of the two tables are RT_ERR_INVALID before any HIP call;
 * rt_last_error_detail() names the check and starts with "rt_reproject_quads".  The tables obey buffers_on_device like every
 * other buffer; host memory is staged, and a table whose count is 0 is not looked at.  Stream and blocking: rt_reproject's rules. */
typedef struct rt_reproject_quad_desc {
    int32_t n_quads, reserved;
    const rt_quad* quads;        /* records the CURRENT frame was rendered with (rt_scene_get_quads) */
    const rt_quad* prev_quads;   /* records the PREVIOUS frame was rendered with, same count and order */
} rt_reproject_quad_desc; /* 24 B */
rt_status rt_reproject_quads(const rt_reproject_desc* d, const rt_reproject_motion_desc* m,
                             const rt_reproject_instance_desc* im, const rt_reproject_quad_desc* qm,
                             int buffers_on_device, void* stream, int blocking);

/* ---- several GPUs of one node from one host thread ----
 * The reference is single-GPU (one render<<<>>> launch, main.cu:707); these entry points are what its host function
 * would call to spread that launch over the N GPUs of a node: rt_init_devices(N) replaces rt_init, rt_multi_create /
 * rt_multi_render / rt_multi_destroy replace rt_scene_create / rt_render / rt_scene_destroy.  The frame is cut into
 * tiles of `tile_rows` rows dealt round-robin to the devices (tile t -> device t % N); every device renders its rows
 * with its own replica of the scene, one ncclGather (rccl.h:745) over xGMI brings the compact row buffers to device 0
 * and a small kernel puts them into the reference's frame layout.  `f` describes the WHOLE frame (its tile_* fields
 * are ignored); fb receives nx*ny*3 floats (host memory, or memory of device 0 when fb_on_device != 0).  The call
 * returns when the frame is complete.  stats: rays / samples summed over the devices, ms_render = host wall time of
 * the frame (render on every device + gather + reassembly + copy; buffer allocation and communicator set-up of a first
 * call excluded), reserved = the slowest device's own render time in microseconds.  By construction pixels are
 * bit-identical to rt_render's on one device -- no ray crosses a device and the per-pixel seed is seed_base + the
 * global pixel index; on one GPU that is tested for every rank's share and for the reassembly at world sizes 2..8
 * (tests/test_gpu_parity.py), with N > 1 devices it is UNVERIFIED ON HARDWARE so far.  On any failure after the frames
 * were enqueued every device is drained (streams synchronised, pending frames closed) before the error is returned. */
typedef struct rt_multi rt_multi;
rt_status rt_init_devices(int n_gpus);
rt_status rt_multi_create(const rt_scene_desc* desc, int n_gpus, rt_multi** out);
rt_status rt_multi_render(rt_multi* m, const rt_frame_desc* f, float* fb, int fb_on_device, int tile_rows, rt_stats* stats);
rt_status rt_multi_destroy(rt_multi* m);
rt_status rt_multi_set_camera(rt_multi* m, const rt_camera* camera, int recalibrate);   /* rt_scene_set_camera on every replica */
rt_status rt_multi_update_spheres(rt_multi* m, const rt_sphere_update* update, int recalibrate);   /* rt_scene_update_spheres, host records, on every replica */
rt_status rt_multi_update_instances(rt_multi* m, const rt_instance_update* update, int recalibrate);   /* rt_scene_update_instances, host records, on every replica */
rt_status rt_multi_update_quads(rt_multi* m, const rt_quad_update* update, int recalibrate);           /* rt_scene_update_quads, host records, on every replica */
int32_t rt_multi_device_count(const rt_multi* m);
/* the row partition rt_multi_render uses: which device renders global row j and at which row of its compact buffer
 * (the inverse of rt_local_to_global_row for tile_first = device, tile_stride = n_gpus) */
rt_status rt_multi_row_owner(int32_t global_row, int32_t tile_rows, int32_t n_gpus, int32_t* device, int32_t* local_row);
/* diagnostics of the multi-GPU path (tests): load RCCL exactly as rt_multi_render would (`library_name` = that name only,
 * null = the usual search) -- a missing library is RT_ERR_HIP with the loader's message, no device needed; and the
 * reassembly step on caller-supplied device buffers, staging[world][max_rows][nx*3] -> frame[ny][nx*3], synchronous. */
rt_status rt_multi_probe_rccl(const char* library_name);
rt_status rt_multi_debug_uninterleave(const float* staging, float* frame, int32_t nx, int32_t ny, int32_t tile_rows, int32_t world, int32_t max_rows);
/* diagnostics of the cost-aware schedule (tests/test_rank.py, tests/rank_expect.py): the device-side ranking and the cost prior
 * run once on caller-supplied HOST buffers -- device memory allocated, the launches rt_render makes enqueued on the null stream,
 * synchronised, copied back, freed -- and what a scene holds of them.  Every argument check runs before any HIP call and is
 * RT_ERR_INVALID with a detail string; the first two need rt_init and no scene.
 * rt_debug_rank: one ranking (tile order, heavy list, tiers).  cost[n_pixels] = the parked costs (bit 31 may be set: a stale list
 * flag), tile_cost[n_tiles], rays = the "rays so far" the thresholds are taken from; params = 20 words:
 *   [0] n_pixels  [1] n_tiles  [2] heavy_cap  [3] max_grid  [4] waves_per_wg  [5] normal_need                       (uint32)
 *   [6] sparse_stride  [7] semi_stride  [8] sparse_percent  [9] sparse_work_percent  [10] tier_possible  [11] tier1_pixels
 *   [12] tier1_depth  [13] tier_wgs_cap  [14] tier_waves_per_main_wg  [15] nx (pixels per local row)  [16] smooth_percent (int32)
 *   [17] heavy_factor  [18] sparse_factor  [19] tier1_factor                                                       (float)
 * Out: tile_order[n_tiles], cost_out[n_pixels] (the costs with this ranking's list flags), heavy_pixels[heavy_cap] (entries the
 * ranking did not write are 0xFFFFFFFF) and info13 = heavy_items, heavy_threshold, tier1_items, tier2_items, tier1_wgs,
 * main_skip_wgs, sparse_wgs, sparse_stride, semi_wgs, semi_stride, threshold1, threshold2, collected.
 * rt_debug_prior: the cost prior of the rows (tile_rows, tile_first, tile_stride) of an nx x ny frame from the calibration
 * costs cal_cost[cal_ny][cal_nx] (row 0 = bottom).  Out: cost_out[local_rows * nx] with local_rows = rt_frame_local_rows,
 * tile_cost_out[((local_rows + 7) / 8) * ((nx + 7) / 8)] and their sum.
 * rt_debug_cal_cost: the calibration costs the scene kept at rt_scene_create, out[*ny][*nx]; cap = the words out holds, at
 * least 64 (the smallest grid is 8 x 8).  A scene that kept none, or a cap below the grid (nx, ny are set), is RT_ERR_INVALID.
 * rt_debug_rank_info: the 13 words, as above, that the last ranking of the scene's last frame left; RT_ERR_INVALID when that
 * frame was not ranked. */
rt_status rt_debug_rank(const uint32_t* cost, const uint32_t* tile_cost, uint64_t rays, const uint32_t* params, uint32_t* tile_order,
                        uint32_t* cost_out, uint32_t* heavy_pixels, uint32_t* info13);
rt_status rt_debug_prior(const uint32_t* cal_cost, int32_t cal_nx, int32_t cal_ny, int32_t nx, int32_t ny, int32_t tile_rows, int32_t tile_first,
                         int32_t tile_stride, uint32_t* cost_out, uint32_t* tile_cost_out, uint64_t* total_out);
rt_status rt_debug_cal_cost(rt_scene* scene, uint32_t* out, int32_t cap, int32_t* nx, int32_t* ny);
rt_status rt_debug_rank_info(rt_scene* scene, uint32_t* out13);
/* diagnostics of the tier kernel's room (tests/test_kernel_matrix.py): what rt_render plans for this scene under the current
 * options -- out4 = [0] 1 when the tier kernel's LDS image fits beside the main kernel (tier 1 and the tail hand-off can run),
 * [1] 1 when that image also holds spheres, materials and textures (which instantiation of the tier kernel runs), [2] the
 * image's bytes, [3] the grid of a tail launch.  All 0 for a scene without tier data or with the tier kernel and the hand-off
 * switched off.  Host only: nothing is launched and the scene is left as it was.  A null scene or a null out4 is
 * RT_ERR_INVALID, and so is a plan rt_render would refuse (a forced lds_mode that does not fit). */
rt_status rt_debug_tier_room(rt_scene* scene, int32_t* out4);
/* diagnostics of the box tests (tests/test_box_tests.py): the walk's three forms of aabb::hit (rt_device_funcs.h: slab_test, the
 * reference's own; slab_test_finite, its equal for rays whose 1/d is finite; slab_test_loose, the walk loop's widened one) run
 * once, one thread per case, on caller-supplied HOST buffers: boxes bmin[n][3] / bmax[n][3], rays origins[n][3] /
 * directions[n][3], windows tmin[n] / tmax[n], and bound3 = the scene bound the widening is taken from (every box coordinate
 * within +-bound3[axis]; finite, not negative).  1/d and the loose terms are set up as the render sets them up.  Out:
 * flags[n][4] = slab_test, slab_test_finite, slab_test_loose, finite_inv (1/d finite and loose_ok: the rays the render gives the
 * two faster forms; for the others their flags are computed all the same and mean nothing).  n = 1 .. 2^24.  Needs rt_init and
 * no scene; every argument check runs before any HIP call; null stream, synchronous. */
rt_status rt_debug_box_tests(int32_t n, const float* bmin, const float* bmax, const float* origins, const float* directions,
                             const float* tmin, const float* tmax, const float* bound3, uint8_t* flags);
/* diagnostics of the exact cheaper arithmetic (tests/test_exact_arith.py): each mode runs a helper of the render
 * path and, inside the kernel, the plain expression it replaces, and compares the two bit for bit.
 *   RT_ARITH_UNIFORM  words 0 .. n - 1 (n = 1 .. 2^32): the one-fma draw against (float)x * 2^-32 + 2^-33; reads no array
 *   RT_ARITH_SIGNED   the same for the rejection loops' 2u - 1
 *   RT_ARITH_LOOSE    the walk loop's loose_setup for rays a[n][3] (origins), b[n][3] (directions) and the scene bound bound3
 *                     (finite, not negative) against its form with selects; compared where finite_inv holds.  n = 1 .. 2^24
 * a, b, path are HOST buffers; the draw modes take them null.  path (RT_ARITH_LOOSE only, may be null) receives finite_inv per
 * ray.  out3 = mismatching cases, index of the first of them (~0 when none), rays with finite_inv (0 for the draw modes).
 * Needs rt_init and no scene; every argument check runs before any HIP call; null stream, synchronous. */
#define RT_ARITH_UNIFORM 0
#define RT_ARITH_SIGNED 1
#define RT_ARITH_LOOSE 2
rt_status rt_debug_arith_tests(int32_t mode, int64_t n, const float* a, const float* b, const float* bound3, uint8_t* path, uint64_t* out3);
/* diagnostics of the third-party part of the numerical contract (tests/test_device_math.py): the render path's own
 * transcendental wrappers of csrc/rt_device_funcs.h, and the plain operations the contract calls IEEE, run on caller-chosen
 * inputs so that their float results can be compared with another maths library's, input by input.
 *   RT_MATH_LOG     cr_log(a)                         RT_MATH_POW5    cr_pow5(a), Schlick's fifth power
 *   RT_MATH_SIN     cr_sin(a)                         RT_MATH_SQRT    sqrtf(a)
 *   RT_MATH_ACOS    cr_acos(a)                        RT_MATH_RCP     1.0f / a
 *   RT_MATH_ATAN2   cr_atan2(a, b)                    RT_MATH_DIV     a / b
 *   RT_MATH_POW     apply_gamma(a, b): b is gamma,    RT_MATH_MULADD  a * b + c as written, built with the library's flags
 *                   1 / gamma is formed as a frame's                  (the contract: the product is rounded, nothing fuses)
 * RT_MATH_SWEEP: the inputs a are the `count` consecutive 32-bit words first, first + 1, ... taken as floats (count = 1 .. 2^32,
 * first + count <= 2^32); b is `operand` (RT_MATH_POW: finite and positive; not read otherwise).  Functions of one input and
 * RT_MATH_POW only.  digests[(count + 2^20 - 1) >> 20] receives one 64-bit digest per block of 2^20 consecutive words counted
 * from `first` (the last block may be short): the sum modulo 2^64, over the block's words w, of mix64(w, r), where r is the bit
 * pattern of the float result, or 0x7FC00000 for every NaN result whatever its sign and payload, and
 *   mix64(w, r):  z = w * 2^32 + r;  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 * in 64-bit unsigned arithmetic (the finaliser of splitmix64).  A sum has no order, so digests of two implementations are equal
 * exactly when -- short of a 2^-64 accident -- every result of the block is; a, b, c and out must be null.
 * RT_MATH_LIST: out[i] = fn(a[i], b[i], c[i]) for i < count (count = 1 .. 2^24; first must be 0, operand is not read).  a, b, c,
 * out are HOST buffers; b and c may be null where fn does not read them; digests must be null.
 * Needs rt_init and no scene; every argument check runs before any HIP call; null stream, synchronous.  Never on a frame's path. */
#define RT_MATH_SWEEP 0
#define RT_MATH_LIST 1
#define RT_MATH_LOG 0
#define RT_MATH_SIN 1
#define RT_MATH_ACOS 2
#define RT_MATH_ATAN2 3
#define RT_MATH_POW 4
#define RT_MATH_POW5 5
#define RT_MATH_SQRT 6
#define RT_MATH_RCP 7
#define RT_MATH_DIV 8
#define RT_MATH_MULADD 9
rt_status rt_debug_math_tests(int32_t form, int32_t fn, uint32_t first, int64_t count, float operand, const float* a, const float* b,
                              const float* c, float* out, uint64_t* digests);
/* The cost map (option cost_map).  The last launches of a ranked frame leave, per local pixel, the rays the
 * pixel cost over all its samples.  A pixel's cost depends on the scene, the camera, the frame geometry and the row partition,
 * not on seed_base or ns, so the next ranked frame of the same scene uses the map once rt_frame_finish has closed the frame
 * that wrote it:
 *   exact -- same nx, ny, tile_rows, tile_first, tile_stride and kernel family, no rt_scene_set_camera / rt_scene_update_spheres
 *            and no rt_set_option / rt_reset_options call since: the frame is ranked on the map and runs as ONE part;
 *   stale -- same geometry, but the camera or a sphere was changed without recalibration, or an option call was made: the map
 *            replaces the calibration frame as the prior of part 1 of the usual two parts.
 * Kernel families whose tier workgroups take main workgroups' slots (scenes that are not spheres-only, or carry noise / image
 * textures, and have tier 1) write the map and do not read it: they measured slower in one part.
 * A change with recalibrate != 0 drops the map; a frame of another geometry does not use it and replaces it.  Unranked
 * frames, windows, adaptive and variance frames neither read nor write it.  Scheduling only: no pixel changes.
 * rt_debug_cost_map: a pending frame is closed first.  info[0] = 0 none / 1 exact / 2 stale (relative to the scene and the options
 * as they are now; 0 while option cost_map is 0), info[1] = the map's nx, info[2] = its local rows, info[3] = the parts the last
 * ranked frame ran as.  out[info[2]][info[1]] receives the map when it is not "none" and cap words hold it; a smaller cap is
 * RT_ERR_INVALID (info is set).  out may be null with cap = 0: info only.
 * rt_debug_set_cost_map: installs in[n] (bit 31 is cleared) as the exact map of the last ranked frame's geometry; n must be that
 * frame's local pixel count.  RT_ERR_INVALID when the scene has rendered no ranked frame or option cost_map is 0. */
rt_status rt_debug_cost_map(rt_scene* scene, uint32_t* out, int64_t cap, int32_t* info4);
rt_status rt_debug_set_cost_map(rt_scene* scene, const uint32_t* in, int64_t n);

/* Tuning knobs (for A/B measurements; defaults are what ships).  Unknown keys
 * return RT_ERR_INVALID.  The knobs are process-wide; rt_reset_options()
 * restores every one of them to the shipped default.  None changes a pixel.
 * Two knobs are read by rt_scene_create and shape the scene it returns: "bvh_collapse" (how the walk array is planned) and
 * "scan_nodes" (a walk array of at most that many nodes is reduced to its leaves, to be scanned in lockstep).  "scan_nodes" is
 * read again by every render's plan, which scans an array of at most that many nodes ("lds_mode" -1) -- whatever the value
 * was at creation, and "lds_mode" 4 scans an array of any size.  A scene created under one value and rendered under another is
 * scanned with its interior nodes still in the array, or walked without them: such a mismatch costs box tests and never pixels
 * (tests/test_kernel_matrix.py). */
rt_status rt_set_option(const char* key, int value);
rt_status rt_reset_options(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_ABI_H */
