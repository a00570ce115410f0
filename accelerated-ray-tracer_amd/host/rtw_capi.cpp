// rtw_capi.cpp -- C entry points of the host scene library (librtw_host.so) for
// tests, bench.py and any non-C++ caller: build a named reference scene on the
// host, flatten it, and hand out the rt_scene_desc the render library takes.
// Pure host code: no HIP here.
#include <cstdio>
#include <memory>
#include <string>

#include "rtw_scenes.h"

namespace {
struct handle {
    std::unique_ptr<rtw::built_scene> scene;
    rtw::flat_scene flat;
    rt_scene_desc desc;
};
thread_local std::string g_err;
}  // namespace

extern "C" {

const char* rtw_last_error(void) { return g_err.c_str(); }

int rtw_scene_count(void) { int n = 0; rtw::scene_names(&n); return n; }
const char* rtw_scene_name(int i) { int n = 0; const char* const* v = rtw::scene_names(&n); return (i >= 0 && i < n) ? v[i] : nullptr; }

// nx/ny <= 0: the reference host function's frame size.  rgb may be null.
void* rtw_scene_build(const char* name, int nx, int ny, const unsigned char* rgb, int w, int h) {
    g_err.clear();
    std::unique_ptr<handle> hd(new handle);
    hd->scene = rtw::build_scene(name ? name : "", nx, ny, rgb, w, h, g_err);
    if (!hd->scene) return nullptr;
    rt_status st = rtw::flatten(hd->scene->world, *hd->scene->cam, hd->flat, g_err,
                                hd->scene->created.data(), (int)hd->scene->created.size());
    if (st != RT_OK) return nullptr;
    hd->desc = hd->flat.desc();
    return hd.release();
}

void rtw_scene_free(void* p) { delete static_cast<handle*>(p); }

const rt_scene_desc* rtw_scene_desc(void* p) { return p ? &static_cast<handle*>(p)->desc : nullptr; }

// out[0..3] = nx, ny, ns, use_gradient_bg ; bg[0..2] ; returns gamma
float rtw_scene_defaults(void* p, int* out4, float* bg3, int* ppm_double_scale) {
    const rtw::built_scene& s = *static_cast<handle*>(p)->scene;
    out4[0] = s.nx; out4[1] = s.ny; out4[2] = s.ns; out4[3] = s.use_gradient_bg;
    bg3[0] = s.background.x(); bg3[1] = s.background.y(); bg3[2] = s.background.z();
    if (ppm_double_scale) *ppm_double_scale = s.ppm_double_scale ? 1 : 0;
    return s.gamma;
}

// per BVH node (depth-first order): creation index of the leaf's object, or -1
int rtw_scene_leaf_order(void* p, int* out, int cap) {
    const rtw::flat_scene& f = static_cast<handle*>(p)->flat;
    int n = (int)f.leaf_order.size();
    for (int i = 0; i < n && i < cap; ++i) out[i] = f.leaf_order[i];
    return n;
}

// the reference's output stage: ASCII P3 to `path` ("-" = stdout)
// flags: bit 0 = the double 255.99 of bouncing_spheres (main.cu:725), bit 1 = binary P6 instead of ASCII P3
int rtw_write_ppm(const char* path, const float* fb, int nx, int ny, int flags) {
    FILE* f = (path && std::string(path) != "-") ? fopen(path, "wb") : stdout;
    if (!f) return -1;
    if (flags & 2) rtw::write_ppm_p6(f, fb, nx, ny, (flags & 1) != 0);
    else rtw::write_ppm_p3(f, fb, nx, ny, (flags & 1) != 0);
    if (f != stdout) fclose(f); else fflush(f);
    return 0;
}

// camera.cuh:59-78 through the host camera class -- the reference's own float arithmetic -- into the ABI's rt_camera: the camera
// a reference scene function would construct from these arguments (lookfrom, lookat, vup: three floats each)
int rtw_camera_init(const float* lookfrom, const float* lookat, const float* vup, float vfov, float aspect, float aperture, float focus_dist,
                    double t0, double t1, rt_camera* out) {
    if (!lookfrom || !lookat || !vup || !out) return -1;
    const rtw::camera cam(rtw::vec3(lookfrom[0], lookfrom[1], lookfrom[2]), rtw::vec3(lookat[0], lookat[1], lookat[2]),
                          rtw::vec3(vup[0], vup[1], vup[2]), vfov, aspect, aperture, focus_dist, t0, t1);
    *out = rtw::camera_desc(cam);
    return 0;
}

// hittable.cuh:89-93 through rotate_y's own float arithmetic: the (sin_t, cos_t) a reference scene function's rotate_y(p, degrees)
// holds, which is what an rt_instance record of that rotation carries
int rtw_rotation(float degrees, float* sin_t, float* cos_t) {
    if (!sin_t || !cos_t) return -1;
    const float rad = degrees * 0.017453292519943295769f;
    *sin_t = sinf(rad);
    *cos_t = cosf(rad);
    return 0;
}

// quad.cuh:29-54 through the host library's own quad constructor: the rt_quad record a reference scene function's
// quad(Q, u, v, material) flattens to -- its D, w and unit normal in the constructor's float arithmetic --, with `mat` as given
// (an index into the scene's materials).  What rt_scene_update_quads takes for a quad that moves or changes shape.
static void quad_record_of(const rtw::quad& q, int mat, rt_quad* out) {
    memset(out, 0, sizeof(*out));
    const rtw::vec3* src[5] = {&q.Q, &q.u, &q.v, &q.w, &q.normal};
    float* dst[5] = {out->Q, out->u, out->v, out->w, out->n};
    for (int k = 0; k < 5; ++k) { dst[k][0] = src[k]->x(); dst[k][1] = src[k]->y(); dst[k][2] = src[k]->z(); }
    out->D = q.D;
    out->mat = mat;
}
int rtw_quad_record(const float* Q, const float* u, const float* v, int mat, rt_quad* out) {
    if (!Q || !u || !v || !out) return -1;
    const rtw::quad q(rtw::vec3(Q[0], Q[1], Q[2]), rtw::vec3(u[0], u[1], u[2]), rtw::vec3(v[0], v[1], v[2]), nullptr);
    quad_record_of(q, mat, out);
    return 0;
}

// quad.cuh:145-162 through the host library's own make_box: the six rt_quad records, in face order, of make_box(a, b, material)
int rtw_box_records(const float* a, const float* b, int mat, rt_quad* out6) {
    if (!a || !b || !out6) return -1;
    std::unique_ptr<rtw::hittable> box(rtw::make_box(rtw::vec3(a[0], a[1], a[2]), rtw::vec3(b[0], b[1], b[2]), nullptr));
    const rtw::compound6* c = dynamic_cast<const rtw::compound6*>(box.get());
    if (!c) return -1;
    int bad = 0;
    for (int f = 0; f < 6; ++f) {
        const rtw::quad* q = dynamic_cast<const rtw::quad*>(c->faces[f]);
        if (q) quad_record_of(*q, mat, out6 + f); else bad = -1;
        delete c->faces[f];                                           // (compound6 does not own its faces)
    }
    return bad;
}

int rtw_load_ppm(const char* path, unsigned char* out, int cap, int* w, int* h) {
    std::vector<unsigned char> px;
    if (!rtw::load_ppm(path, px, *w, *h)) return -1;
    if (out && (int)px.size() <= cap) memcpy(out, px.data(), px.size());
    return (int)px.size();
}

}  // extern "C"
