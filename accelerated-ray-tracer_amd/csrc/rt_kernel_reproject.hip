// rt_kernel_reproject.hip -- the current frame blended into the reprojected history of the previous frame, as include/rt_abi.h
// ("temporal reprojection" and its three extensions) spells it out, gfx950.  The arithmetic is the contract's, statement by
// statement (-ffp-contract=off: no FMA is formed).
//
// One kernel template, one lane per pixel, workgroups of 256 threads on 16x16 pixel tiles.  Inside a tile the lanes run row-major
// (lane & 15 across, four rows per wave): every planar access of a wave -- the pixel's own colour, depth, alpha, normal and
// ids, and the three outputs -- is then four runs of 16 consecutive pixels (64 B of a scalar plane, 192 B of an rgb plane),
// and since a reprojection is locally close to a translation the four taps of those lanes fall on neighbouring runs of at
// most six rows of the previous frame, which the next wave of the tile (four rows further up) mostly shares through L1/L2.
// There is no LDS staging: where a tile's taps land is data (the depth), so a window cannot be fetched before it is known, and
// the footprint of a tile is already about one tile of each plane.
//
// Forms.  The kernel is specialised on (normal test, id test, motion output), so that a guide that is off costs neither loads
// nor registers, and on its optional second argument, the tables of the follow step (rt_device.h):
//   static     no second argument: rt_reproject, eight instantiations.  Steps 1 to 4 and nothing else.
//   spheres    rt_reproject_follow_params: a surface pixel on a sphere, or in a medium a sphere bounds, whose record changed is
//              carried back to where that surface point was.
//   instances  ..._follow_instance_params: in front of that, a pixel on an instance (inst[p], or the boundary of its medium) whose
//              record changed has its point and its normal taken through the current record's world -> object map and the
//              previous record's object -> world map; a tap must also show the pixel's inst (4.19).
//   quads      ..._follow_quad_params: in front of both, a pixel on a quad of the tables (a face of a box is one) whose Q, u or v
//              changed goes into object space by its instance record, if it has one, onto the previous record's plane by its
//              planar coordinates in the current one, and out by the previous instance record; its normal becomes the previous
//              record's n on the side the pixel saw (4.21).
// The follow forms always test ids: four instantiations each, twenty in all.  The follow step is written in the kernel's body, not
// as helper functions: its prim decode, its sphere carry and its instance and quad block stand there once each, and `if constexpr`
// on the argument's type leaves a form only its own paths.  The block's y-rotations (point and normal, in and out) are spelled out:
// as functions or lambdas, in every spelling tried, they cost the instance kernels without normals two to four VGPRs and changed
// which multiplies are packed (profiles/reproject_shared_isa.txt); as text all twenty kernels are what they were.
//
// Memory phases.  What a lane waits for is the latency of dependent round trips, not bandwidth: per pixel it reads up to 40 B of
// the current frame and four taps of up to 44 B, and writes up to 24 B.  Phase one is the pixel's own data.  The follow forms add
// one phase: at most one medium record, then the records of both frames -- two 32-byte sphere records, or two 32-byte instance
// records, or two 80-byte quad records, or those four -- issued together ahead of every test on them; the lanes of one object
// share their lines.  The last phase is the taps: the loads of all four are issued before the first is looked at.
//
// Bounds.  The pixel's own index is tested against the frame before any address is formed.  A tap address is formed only from
// x0, y0 after the float comparisons -1 <= x0 <= nx - 1, -1 <= y0 <= ny - 1 (false for a NaN) have passed and after the tap's
// integer coordinates have compared as inside the image (unsigned: -1 wraps and compares as outside).  Every plane of the
// previous frame holds ny * nx pixels, prev_inst among them, so every load of a tap that is inside the image is inside its buffer,
// whatever the other buffers hold; a tap outside the image reads at the pixel's own index instead and is not counted.  The
// follow step forms four more kinds of address from data, each after an unsigned comparison with the table's count:
// media[index] after index < n_media, spheres[k] / prev_spheres[k] after k < n_spheres, instances[i] / prev_instances[i] after
// i < n_instances, quads[g] / prev_quads[g] after g < n_quads.  What the records hold is only ever arithmetic; a medium's
// boundary is decoded into an index that passes the same comparisons; flag bits are only tested.
#include <type_traits>

#include "rt_device.h"
#include "rt_launch.h"

namespace {

constexpr int TILE = RT_REPROJECT_TILE;

constexpr unsigned NONE = 0xFFFFFFFFu, INDEX = 0x0FFFFFFFu;   // no record; the index bits of an RT_PRIM_REF

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// the kernel's optional second argument, and what its type says the follow step looks for
template <class F> __device__ __forceinline__ const F& tables(const F& f) { return f; }
template <class... Follow> constexpr bool follows_instances = (std::is_base_of_v<rt_reproject_follow_instance_params, Follow> || ...);
template <class... Follow> constexpr bool follows_quads = (std::is_base_of_v<rt_reproject_follow_quad_params, Follow> || ...);

// One lane per pixel; the body is the contract's steps in order.  <NRM, IDS, MOT>: the normal test, the id test, the motion output.
// Follow: nothing (rt_reproject), or the tables of the follow step as a second argument; a follow form reads prim[p] whatever IDS
// says, an instance form also inst[p] and, among the taps, prev_inst.
template <bool NRM, bool IDS, bool MOT, class... Follow>
__global__ __launch_bounds__(RT_REPROJECT_THREADS) void rt_reproject_kernel(rt_reproject_params rp, Follow... follow) {
    constexpr bool FOL = sizeof...(Follow) > 0, INS = follows_instances<Follow...>, QUA = follows_quads<Follow...>;
    const int tid = threadIdx.x;
    const int nx = rp.nx, ny = rp.ny;
    const unsigned by = blockIdx.x / (unsigned)rp.tiles_x, bx = blockIdx.x - by * (unsigned)rp.tiles_x;
    const unsigned i = bx * TILE + (tid & (TILE - 1)), j = by * TILE + (tid / TILE);
    if (i >= (unsigned)nx || j >= (unsigned)ny) return;
    const size_t p = (size_t)j * nx + i;

    const float cr = rp.color[3 * p], cg = rp.color[3 * p + 1], cb = rp.color[3 * p + 2];
    const float al = rp.alpha[p], dep = rp.depth[p];
    float npx = 0.f, npy = 0.f, npz = 0.f;
    if (NRM) { npx = rp.normal[3 * p]; npy = rp.normal[3 * p + 1]; npz = rp.normal[3 * p + 2]; }
    int32_t idp = 0;
    if (IDS || FOL) idp = rp.prim[p];
    int32_t insp = 0;
    if constexpr (INS) insp = tables(follow...).inst[p];

    // 1. the pixel's centre ray and its world point (or, for sky, its direction: a point at infinity)
    const float fi = (float)(int)i, fj = (float)(int)j, fnx = (float)nx, fny = (float)ny;
    const float s = (fi + 0.5f) / fnx, t = (fj + 0.5f) / fny;
    float q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = ((rp.lower_left[c] + s * rp.horizontal[c]) + t * rp.vertical[c]) - rp.origin[c];
    const bool surface = al >= rp.alpha_min;
    if (surface) {
        const float z = dep / al;
        float P[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            P[c] = rp.origin[c] + z * q[c];
            q[c] = P[c] - rp.prev_origin[c];
        }
        // 1-follow. a surface point on something that moved goes back to where it was, its normal with it
        if constexpr (FOL) {
            const rt_reproject_follow_params& fp = tables(follow...);
            // 1a. what the pixel's prim says it follows.  k: the sphere it shows, or the one that bounds the medium it shows.  ii
            // (the instance forms): inst[p], or without one the instance that bounds its medium.  At most one medium record is
            // loaded, after index < n_media compared unsigned; of what it holds only the kind is tested and the index bits kept,
            // and those pass the tables' own comparisons before an address is formed.
            unsigned k = NONE, ii = NONE;
            if (INS && insp >= 0) ii = (unsigned)insp;
            if (idp >= 0) {
                const unsigned kind = (unsigned)idp >> 28, index = (unsigned)idp & INDEX;
                if (kind == (unsigned)RT_PRIM_SPHERE) {
                    k = index;
                } else if (kind == (unsigned)RT_PRIM_MEDIUM && index < (unsigned)fp.n_media) {
                    const int32_t b = fp.media[index].boundary;
                    if (b >= 0 && ((unsigned)b >> 28) == (unsigned)RT_PRIM_SPHERE) k = (unsigned)b & INDEX;
                    if (INS && insp < 0 && b >= 0 && ((unsigned)b >> 28) == (unsigned)RT_PRIM_INSTANCE) ii = (unsigned)b & INDEX;
                }
            }
            if constexpr (INS) {
                // 1a'. an instance in range takes the pixel: the sphere steps are skipped.
                const rt_reproject_follow_instance_params& ip = tables(follow...);
                bool ipath = ii < (unsigned)ip.n_instances;
                // 1a''. which quad: the pixel's own prim, when the tables hold it and its inst is none or in range (a quad's prim
                // is no medium, so ii is inst[p] or none here).  Such a pixel takes this block with or without an instance.
                bool qpath = false;
                unsigned g = 0;
                if constexpr (QUA) {
                    if (idp >= 0 && ((unsigned)idp >> 28) == (unsigned)RT_PRIM_QUAD) {
                        g = (unsigned)idp & INDEX;
                        qpath = g < (unsigned)tables(follow...).n_quads && (insp < 0 || ipath);
                    }
                }
                if (ipath || qpath) {
                    k = NONE;
                    // 1b'. both records' loads are issued together; only their floats and flag bits are used
                    rt_instance I, J;
                    if constexpr (QUA) {   // 1b''. ... and with them the two quad records of a quad pixel
                        I.sin_t = I.cos_t = I.offset[0] = I.offset[1] = I.offset[2] = 0.f; I.flags = 0;
                        J = I;
                        if (ipath) { I = ip.instances[ii]; J = ip.prev_instances[ii]; }
                    } else {
                        I = ip.instances[ii]; J = ip.prev_instances[ii];
                    }
                    float GQ[3] = {}, Gu[3] = {}, Gv[3] = {}, Gw[3] = {}, Gn[3] = {}, HQ[3] = {}, Hu[3] = {}, Hv[3] = {}, Hn[3] = {};
                    bool qmoved = false;
                    if constexpr (QUA) {
                        if (qpath) {
                            const rt_quad* G = tables(follow...).quads + g;
                            const rt_quad* H = tables(follow...).prev_quads + g;
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                GQ[c] = G->Q[c]; Gu[c] = G->u[c]; Gv[c] = G->v[c]; Gw[c] = G->w[c]; HQ[c] = H->Q[c]; Hu[c] = H->u[c]; Hv[c] = H->v[c];
                                if (NRM) { Gn[c] = G->n[c]; Hn[c] = H->n[c]; }
                            }
#pragma unroll
                            for (int c = 0; c < 3; ++c) qmoved = qmoved || GQ[c] != HQ[c] || Gu[c] != Hu[c] || Gv[c] != Hv[c];
                        }
                    }
                    bool moved = I.sin_t != J.sin_t || I.cos_t != J.cos_t || I.offset[0] != J.offset[0] || I.offset[1] != J.offset[1] ||
                                 I.offset[2] != J.offset[2] || I.flags != J.flags;
                    if constexpr (QUA) moved = moved || qmoved;
                    if (moved) {   // 1c'. world -> object by the current record, object -> previous world by the previous one
                        float A[3] = {P[0], P[1], P[2]};
                        if (I.flags & RT_INST_TRANSLATE) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) A[c] = P[c] - I.offset[c];
                        }
                        float B[3] = {A[0], A[1], A[2]};
                        if (I.flags & RT_INST_ROTATE_Y) {
                            B[0] = I.cos_t * A[0] - I.sin_t * A[2];
                            B[2] = I.sin_t * A[0] + I.cos_t * A[2];
                        }
                        if constexpr (QUA) {
                            if (qmoved) {   // 1c''. onto the previous record's plane by the planar coordinates in the current one
                                const float h[3] = {B[0] - GQ[0], B[1] - GQ[1], B[2] - GQ[2]};
                                const float x[3] = {h[1] * Gv[2] - h[2] * Gv[1], h[2] * Gv[0] - h[0] * Gv[2], h[0] * Gv[1] - h[1] * Gv[0]};
                                const float y[3] = {Gu[1] * h[2] - Gu[2] * h[1], Gu[2] * h[0] - Gu[0] * h[2], Gu[0] * h[1] - Gu[1] * h[0]};
                                const float alpha = dot3(Gw[0], Gw[1], Gw[2], x[0], x[1], x[2]);
                                const float beta = dot3(Gw[0], Gw[1], Gw[2], y[0], y[1], y[2]);
#pragma unroll
                                for (int c = 0; c < 3; ++c) B[c] = (HQ[c] + alpha * Hu[c]) + beta * Hv[c];
                            }
                        }
                        float Cc[3] = {B[0], B[1], B[2]};
                        if (J.flags & RT_INST_ROTATE_Y) {
                            Cc[0] = J.cos_t * B[0] + J.sin_t * B[2];
                            Cc[2] = J.cos_t * B[2] - J.sin_t * B[0];
                        }
                        if (J.flags & RT_INST_TRANSLATE) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) Cc[c] = Cc[c] + J.offset[c];
                        }
#pragma unroll
                        for (int c = 0; c < 3; ++c) q[c] = Cc[c] - rp.prev_origin[c];
                        if (NRM) {   // the normal turns with the surface: the same two rotations, no translation
                            float bx = npx, bz = npz;
                            if (I.flags & RT_INST_ROTATE_Y) {
                                bx = I.cos_t * npx - I.sin_t * npz;
                                bz = I.sin_t * npx + I.cos_t * npz;
                            }
                            if constexpr (QUA) {
                                if (qmoved) {   // the previous record's normal, on the side the pixel saw and of its length
                                    const float side = dot3(bx, npy, bz, Gn[0], Gn[1], Gn[2]);
                                    bx = side * Hn[0]; npy = side * Hn[1]; bz = side * Hn[2];
                                }
                            }
                            npx = bx; npz = bz;
                            if (J.flags & RT_INST_ROTATE_Y) {
                                npx = J.cos_t * bx + J.sin_t * bz;
                                npz = J.cos_t * bz - J.sin_t * bx;
                            }
                        }
                    }
                }
            }
            if (k < (unsigned)fp.n_spheres) {
                // 1b. both records' loads are issued together (one round trip), ahead of the taps' phase
                const rt_sphere S = fp.spheres[k], T = fp.prev_spheres[k];
                float cc[3], cp[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    cc[c] = S.c0[c] + fp.time * S.vel[c];
                    cp[c] = T.c0[c] + fp.prev_time * T.vel[c];
                }
                const bool moved = cc[0] != cp[0] || cc[1] != cp[1] || cc[2] != cp[2] || S.radius != T.radius;
                if (moved) {   // 1c. the carry: the similarity that takes the sphere's surface onto its previous self
                    const float ratio = T.radius / S.radius;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float Pp = cp[c] + (P[c] - cc[c]) * ratio;
                        q[c] = Pp - rp.prev_origin[c];
                    }
                }
            }
        }
    }

    // 2. into the previous camera
    const float a = dot3(rp.m[0], rp.m[1], rp.m[2], q[0], q[1], q[2]);
    const float b = dot3(rp.m[3], rp.m[4], rp.m[5], q[0], q[1], q[2]);
    const float c = dot3(rp.m[6], rp.m[7], rp.m[8], q[0], q[1], q[2]);
    float mx = 0.f, my = 0.f;
    float W = 0.f, Cr = 0.f, Cg = 0.f, Cb = 0.f, L = 0.f;
    if (a > 0.f) {
        const float x = (b / a) * fnx - 0.5f, y = (c / a) * fny - 0.5f;
        mx = x - fi;
        my = y - fj;
        const float x0 = floorf(x), y0 = floorf(y);
        if (rp.history && x0 >= -1.f && x0 <= (float)(nx - 1) && y0 >= -1.f && y0 <= (float)(ny - 1)) {
            // ((float)(n - 1) rounds up to 2^31 for the largest widths: the conversion stays defined and the tap is outside)
            const int ix = x0 >= 2147483648.f ? 2147483647 : (int)x0, iy = y0 >= 2147483648.f ? 2147483647 : (int)y0;
            const float fx = x - x0, fy = y - y0;
            const float gx = 1.f - fx, gy = 1.f - fy;
            const float w4[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
            // 3. the four taps.  Their loads are issued together, ahead of every test on what they return: one memory round
            // trip per pixel, where load-test-load tap by tap takes four (measured 1.7 x slower).  A tap outside the image
            // reads at the pixel's own index p instead (an address that depends on no data) and is not counted.
            bool inside[4];
            size_t o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned qx = (unsigned)ix + (unsigned)(k & 1), qy = (unsigned)iy + (unsigned)(k >> 1);
                inside[k] = qx < (unsigned)nx && qy < (unsigned)ny;
                o[k] = inside[k] ? (size_t)qy * nx + qx : p;
            }
            float hl[4], pa[4], pd[4], hr[4], hg[4], hb[4], nqx[4] = {}, nqy[4] = {}, nqz[4] = {};
            int32_t idq[4] = {}, insq[4] = {};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                hl[k] = rp.history_len[o[k]]; pa[k] = rp.prev_alpha[o[k]]; pd[k] = rp.prev_depth[o[k]];
                hr[k] = rp.history[3 * o[k]]; hg[k] = rp.history[3 * o[k] + 1]; hb[k] = rp.history[3 * o[k] + 2];
                if (NRM) { nqx[k] = rp.prev_normal[3 * o[k]]; nqy[k] = rp.prev_normal[3 * o[k] + 1]; nqz[k] = rp.prev_normal[3 * o[k] + 2]; }
                if (IDS) idq[k] = rp.prev_prim[o[k]];
                if constexpr (INS) insq[k] = tables(follow...).prev_inst[o[k]];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bool counts = inside[k] && hl[k] > 0.f;
                if (surface) {
                    const float zq = pd[k] / pa[k];
                    counts = counts && pa[k] >= rp.alpha_min && fabsf(zq - a) <= rp.depth_tol * fmaxf(zq, a);
                    if (NRM) counts = counts && dot3(npx, npy, npz, nqx[k], nqy[k], nqz[k]) >= rp.normal_min;
                } else {
                    counts = counts && pa[k] < rp.alpha_min;
                }
                if (IDS) counts = counts && idp == idq[k];
                if constexpr (INS) counts = counts && insp == insq[k];
                if (counts) {
                    const float w = w4[k];
                    W = W + w;
                    Cr = Cr + w * hr[k];
                    Cg = Cg + w * hg[k];
                    Cb = Cb + w * hb[k];
                    L = L + w * hl[k];
                }
            }
        }
    }

    // 4. blend
    float outr = cr, outg = cg, outb = cb, len = 1.f;
    if (W > 0.f) {
        const float hr = Cr / W, hg = Cg / W, hb = Cb / W;
        const float n = fminf(L / W, rp.max_history);
        len = n + 1.f;
        const float g = 1.f / len;
        outr = hr + (cr - hr) * g;
        outg = hg + (cg - hg) * g;
        outb = hb + (cb - hb) * g;
    }
    rp.out[3 * p] = outr;
    rp.out[3 * p + 1] = outg;
    rp.out[3 * p + 2] = outb;
    rp.out_len[p] = len;
    if (MOT) {
        rp.motion[2 * p] = mx;
        rp.motion[2 * p + 1] = my;
    }
}

template <bool NRM, bool IDS, bool MOT, class... Follow>
hipError_t launch(const rt_reproject_params& rp, hipStream_t st, const Follow&... follow) {
    const unsigned tiles_y = ((unsigned)rp.ny + TILE - 1) / TILE;
    return rt_launch_kernel(rt_reproject_kernel<NRM, IDS, MOT, Follow...>, dim3(RT_REPROJECT_THREADS), dim3((unsigned)rp.tiles_x * tiles_y), 0, st, rp, follow...);
}
template <bool IDS, class... Follow>
hipError_t launch_flags(bool normals_on, bool motion_on, const rt_reproject_params& rp, hipStream_t st, const Follow&... follow) {
    if (normals_on) return motion_on ? launch<true, IDS, true>(rp, st, follow...) : launch<true, IDS, false>(rp, st, follow...);
    return motion_on ? launch<false, IDS, true>(rp, st, follow...) : launch<false, IDS, false>(rp, st, follow...);
}

}  // namespace

// The kernel of a form takes the slice of `qp` that is the form's own argument: none, its sphere part, its instance part, all of it.
// The follow forms always test ids (their entries require prim and prev_prim; without a history no tap is read).
hipError_t rt_launch_reproject(rt_reproject_form form, bool normals_on, bool ids_on, bool motion_on, const rt_reproject_params& rp,
                               const rt_reproject_follow_quad_params& qp, hipStream_t st) {
    switch (form) {
    case RT_REPROJECT_STATIC: return ids_on ? launch_flags<true>(normals_on, motion_on, rp, st) : launch_flags<false>(normals_on, motion_on, rp, st);
    case RT_REPROJECT_SPHERES: return launch_flags<true, rt_reproject_follow_params>(normals_on, motion_on, rp, st, qp);
    case RT_REPROJECT_INSTANCES: return launch_flags<true, rt_reproject_follow_instance_params>(normals_on, motion_on, rp, st, qp);
    case RT_REPROJECT_QUADS: return launch_flags<true, rt_reproject_follow_quad_params>(normals_on, motion_on, rp, st, qp);
    }
    return hipErrorInvalidValue;
}
