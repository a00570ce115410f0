// rt_refit_host.h -- the host half of rt_scene_update_spheres (include/rt_abi.h): the box rule, the checks of
// an update and the refit of a node array in the description's link encoding.  Plain C++ with no HIP call, so that
// rt_refit_nodes needs no device and the same text compiles into a stand-alone host program; rt_kernel_refit.hip takes the
// box rule from here too, so host and device cannot drift apart.
#pragma once
#include <math.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rt_abi.h"

#if defined(__HIPCC__)
#define RT_REFIT_HD __host__ __device__
#else
#define RT_REFIT_HD
#endif

namespace rt_refit {

// The box rule (rt_abi.h): r = |radius|, a = c0 + 0 vel, b = c0 + 1 vel, lo = min(a - r, b - r), hi = max(a + r, b + r), every
// operation a binary32 one rounded once (the build has contraction off; a contracted form would round the same: 0 vel and
// 1 vel are exact).  For radius >= 0 this is the host library's sphere constructors value for value (host/rtw.cpp).
RT_REFIT_HD inline void sphere_box(const rt_sphere& s, float lo[3], float hi[3]) {
    const float r = fabsf(s.radius);
    for (int c = 0; c < 3; ++c) {
        const float a = s.c0[c] + 0.0f * s.vel[c];
        const float b = s.c0[c] + 1.0f * s.vel[c];
        lo[c] = fminf(a - r, b - r);
        hi[c] = fmaxf(a + r, b + r);
    }
}

// what the checks allow of a record: every float finite, mat one of the scene's materials
RT_REFIT_HD inline bool record_ok(const rt_sphere& s, int32_t n_materials) {
    // (x - x == 0 exactly for finite x only; written without isfinite so that host and device share the text)
    bool finite = s.radius - s.radius == 0.0f;
    for (int c = 0; c < 3; ++c) finite = finite && (s.c0[c] - s.c0[c] == 0.0f) && (s.vel[c] - s.vel[c] == 0.0f);
    return finite && s.mat >= 0 && s.mat < n_materials;
}

// The sphere a leaf's box follows: the leaf's own sphere, or the sphere that is the boundary of the leaf's constant_medium
// directly; -1 for every other leaf (quads, boxes, instances, media bounded by anything else), which keeps its box.
inline int32_t leaf_sphere(int32_t prim, const rt_medium* media, int32_t n_media, int32_t n_spheres) {
    if (prim < 0) return -1;
    if (RT_PRIM_KIND(prim) == RT_PRIM_MEDIUM) {
        const int m = RT_PRIM_INDEX(prim);
        if (m >= n_media) return -1;
        prim = media[m].boundary;
        if (prim < 0) return -1;
    }
    if (RT_PRIM_KIND(prim) != RT_PRIM_SPHERE) return -1;
    const int i = RT_PRIM_INDEX(prim);
    return i < n_spheres ? i : -1;
}

// per sphere: whether it is the child of an instance (its box then follows the instance's rule, which an update does not redo)
inline std::vector<char> instanced_spheres(const rt_instance* instances, int32_t n_instances, int32_t n_spheres) {
    std::vector<char> under((size_t)(n_spheres > 0 ? n_spheres : 0), 0);
    for (int i = 0; i < n_instances; ++i) {
        const int32_t c = instances[i].child;
        if (c >= 0 && RT_PRIM_KIND(c) == RT_PRIM_SPHERE && RT_PRIM_INDEX(c) < n_spheres) under[(size_t)RT_PRIM_INDEX(c)] = 1;
    }
    return under;
}

// The refusals of an update (rt_abi.h), none of which needs a device: null or empty text = fine.  host_records: the records
// can be read here (their values are checked); device-resident records are checked by the leaf kernel instead.
inline std::string check_update(const rt_sphere_update* u, bool host_records, int32_t n_spheres, int32_t n_materials,
                                const std::vector<char>& instanced) {
    if (!u) return "null update";
    if (u->count < 0) return "count is negative";
    if (u->count == 0) return "";
    if (!u->spheres) return "null sphere records";
    if (u->count > n_spheres) return "more records than the scene has spheres (an index is out of range or appears twice)";
    std::vector<char> seen((size_t)n_spheres, 0);
    for (int32_t k = 0; k < u->count; ++k) {
        const long long i = u->indices ? (long long)u->indices[k] : (long long)u->first + k;
        if (i < 0 || i >= n_spheres) return "sphere index out of range";
        if (seen[(size_t)i]) return "a sphere index appears twice";
        seen[(size_t)i] = 1;
        if (instanced[(size_t)i]) return "an updated sphere is the child of an instance (its box follows the instance's rule)";
        if (host_records) {
            const rt_sphere& s = u->spheres[k];
            const rt_sphere geometry = {{s.c0[0], s.c0[1], s.c0[2]}, s.radius, {s.vel[0], s.vel[1], s.vel[2]}, 0};
            if (!record_ok(geometry, 1)) return "a sphere record has a non-finite c0, vel or radius";
            if (s.mat < 0 || s.mat >= n_materials) return "sphere material out of range";
        }
    }
    return "";
}

// Refit of a node array in the description's encoding (skip = index of the next node when the box is missed, prim < 0 =
// interior, depth-first pre-order): the leaves whose sphere is marked in `moved` take the box rule's box of spheres[...],
// then every interior node becomes the float min / max union of its children's boxes, children before parents (a node's
// children are i + 1 and the nodes its skip chain reaches below skip[i]).  Link words are not written.
inline void refit_nodes(rt_node* nodes, int32_t n, const rt_sphere* spheres, int32_t n_spheres, const rt_medium* media, int32_t n_media,
                        const std::vector<char>& moved) {
    for (int32_t i = 0; i < n; ++i) {
        const int32_t si = leaf_sphere(nodes[i].prim, media, n_media, n_spheres);
        if (si >= 0 && moved[(size_t)si]) sphere_box(spheres[si], nodes[i].bmin, nodes[i].bmax);
    }
    for (int32_t i = n - 1; i >= 0; --i) {
        if (nodes[i].prim >= 0) continue;
        bool first = true;
        for (int32_t j = i + 1; j < nodes[i].skip && j < n; j = nodes[j].skip) {
            for (int c = 0; c < 3; ++c) {
                nodes[i].bmin[c] = first ? nodes[j].bmin[c] : fminf(nodes[i].bmin[c], nodes[j].bmin[c]);
                nodes[i].bmax[c] = first ? nodes[j].bmax[c] : fmaxf(nodes[i].bmax[c], nodes[j].bmax[c]);
            }
            first = false;
        }
    }
}

}  // namespace rt_refit
