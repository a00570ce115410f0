// main.cpp -- drop-in for the reference's src/main.cu host side: renders one of
// the reference's scenes on an MI355X through the C ABI and writes an ASCII
// PPM (P3) to stdout, progress and timing to stderr (main.cu:668-669,712,
// 715-727).  The reference selects the scene with an integer literal in
// `switch (10)` (main.cu:1309); here it is a flag, and with no flags the
// program renders what the reference's main() does not fall through to:
// `--scene bouncing` is case 1, `--scene final` case 9.
//
//   rayTracer [--scene NAME] [--nx W --ny H] [--ns SPP] [--seed S]
//             [--texture file.ppm] [--device N] [--gpus N] [--p6] [--progressive K] [--adaptive T [--min-spp M]] [--aov PREFIX] [--denoise [K] [--denoise-variance [B]]] [--list]
//             [--upscale F]
//             [--aov-through PREFIX] [--through-bounces N] [--through-fuzz F] [--denoise-through]
//             [--orbit FRAMES DEGREES --out PREFIX [--temporal] [--bounce HEIGHT] [--spin DEGREES [--follow-instances]]
//                                                  [--grow AMOUNT [--follow-quads]]]
//
// --orbit FRAMES DEGREES renders a turntable: FRAMES frames of one device scene, the scene's lookfrom rotated about the vertical
// axis through its lookat in equal steps of DEGREES / FRAMES (frame k at k steps; every other camera argument kept), each
// through rt_scene_set_camera -- one rt_scene_create for the whole sequence.  The images go to PREFIX_000.ppm, PREFIX_001.ppm,
// ... (--out PREFIX is required; nothing is written to stdout).  With --temporal every image is the temporal accumulation of
// the frames so far (rt_reproject with the binding's defaults, normals and ids on, guided by rt_render_aov at min(ns, 16)
// samples): the frames are rendered at gamma 1 and the gamma is applied on the host afterwards, as --denoise does.  Not with
// --gpus > 1, --progressive, --adaptive, --denoise, --aov or --aov-through.
// --bounce HEIGHT (only with --orbit; HEIGHT finite and >= 0; DEGREES may be 0 for a still camera) also moves the small spheres:
// before frame k every sphere i of the description whose radius is in (0, 0.5) gets
//   c0.y = (float)((double)base_y + HEIGHT * fabs(sin(pi * ((double)k / FRAMES + 0.61803398875 * i))))
// (in double, libm's sin) through rt_scene_update_spheres.  With --temporal the accumulation follows them (rt_reproject_moving
// with the records of this frame and of the previous one).  A scene with instances is refused: some of its spheres cannot move.
// --spin DEGREES (only with --orbit; DEGREES finite) turns the rotated instances: before frame k every instance of the description
// with RT_INST_ROTATE_Y takes the angle  atan2((double)sin_t, (double)cos_t) + k * DEGREES * pi / 180  of its flattened record,
// sin and cos evaluated in double and rounded to float, through rt_scene_update_instances.  A scene without a rotated instance
// is refused, and so is --temporal: the reprojection does not follow a moved instance.
// --follow-instances (only with --orbit ... --spin) turns the accumulation on as --temporal does and lets it follow the turning
// instances: rt_render_aov's inst plane is kept with each frame, the instance records are read back after the update
// (rt_scene_get_instances), and from the second frame on the history comes from rt_reproject_instances with the records and inst
// planes of this frame and of the previous one (no sphere table, the scene's media, the binding's default times).
// --grow AMOUNT (only with --orbit; AMOUNT finite, |AMOUNT| < 1) changes the height of the boxes: before frame k every box of the
// description is rebuilt by the host library's make_box(a, b', material of its first face) and sent through
// rt_scene_update_quads, where a and b are the per-axis min / max over the corners Q, Q + u, Q + v, (Q + u) + v of its six
// original faces, b' = b on x and z and
//   b'.y = (float)((double)a.y + ((double)b.y - a.y) * (1 + AMOUNT * sin(2 pi k / FRAMES)))
// (in double, libm's sin).  A scene without a box is refused, and so is --temporal: the plain accumulation does not follow a box
// that changes size.
// --follow-quads (only with --orbit ... --grow) turns the accumulation on and lets it follow the faces: the quad records are read
// back after the update (rt_scene_get_quads), the inst plane and the instance records are kept as --follow-instances keeps them,
// and from the second frame on the history comes from rt_reproject_quads.  It combines with --spin ... --follow-instances.
//
// --denoise [K] filters the frame with rt_denoise (K iterations, 5 when K is left out; the binding's other defaults): the frame
// is rendered at gamma 1, the feature pass (albedo, normal, depth at min(ns, 16) samples) guides the filter, and the frame's
// gamma is applied on the host afterwards -- as powf(c, 1 / gamma) per channel, so the image is not rt_render's bit for bit
// even where the filter changes nothing.  With --aov PREFIX the unfiltered frame is written to PREFIX_noisy.ppm as well.  Works
// with --adaptive; not with --progressive or --gpus > 1.
// --upscale F (F in 2..8; --nx and --ny, which stay the size of the image, must be multiples of it) traces the paths at
// nx/F x ny/F and rebuilds the image with rt_upscale (the binding's defaults): the coarse frame is rendered at gamma 1 with --ns
// samples -- a coarse frame has 1 / F^2 of the pixels, so equal path cost with a full render at n samples is --ns n F^2 --, the
// feature pass runs on both grids at min(ns, 16) samples, --denoise [K], when given, filters the coarse frame with its own
// guides before the upscale, and the frame's gamma is applied on the host afterwards, as --denoise does.  Not with --gpus > 1,
// --progressive, --adaptive, --orbit, --aov, --aov-through, --denoise-variance or --denoise-through.
// --denoise-variance [B] (needs --denoise) makes the filter variance-guided (rt_denoise_variance, the binding's defaults): the
// frame comes from rt_render_variance with B batches -- when B is left out, the largest divisor of --ns in 2..16 (an --ns without one is refused) -- and
// its per-pixel variance takes the colour factor's place.  --ns must be a multiple of B (2..64).  Not with --adaptive.
// --aov PREFIX also writes the frame's feature buffers (rt_render_aov, same camera, seed and sample count) next to the image,
// in the image's PPM flavour: PREFIX.albedo.ppm, PREFIX.normal.ppm (0.5 n + 0.5) and PREFIX.depth.ppm (grey, the ray parameter
// t over the frame's largest).  Not with --gpus > 1.
// --aov-through PREFIX writes the same three files from rt_render_aov_through: the features of the first non-specular surface
// behind glass and in mirrors, and PREFIX.through.ppm (grey: the share of the pixel's samples that followed a bounce).
// --through-bounces N (0..16, default 8) and --through-fuzz F (>= 0, default 0: perfect mirrors only) are the chain's limits.
// --denoise-through (needs --denoise) takes the filter's guides from that pass instead of rt_render_aov.  Not with --gpus > 1.

// --adaptive T renders with adaptive sampling (rt_render_adaptive): each pixel stops at the first checkpoint M * 2^k where its
// average moved by at most T * (brightness + 0.01) since the previous one, and at --ns (= max_spp) otherwise.  M defaults to
// the smallest checkpoint of --ns that is even and >= 16.  Not with --progressive or --gpus > 1.
// --gpus N (N > 1) spreads the frame over the first N GPUs of the node: interleaved 4-row tiles, one scene replica
// per device, one RCCL gather to device 0 (rt_multi_*, include/rt_abi.h).  The PPM is byte-identical for every N by construction (global per-pixel seeds,
// no cross-device rays); verified on one GPU for N = 1 and for every rank's share, not yet on N > 1 hardware.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt_abi.h"
#include "rtw_scenes.h"

extern "C" int rtw_box_records(const float* a, const float* b, int mat, rt_quad* out6);   // librtw_host: the six faces of make_box(a, b)

// checkCudaErrors (main.cu:23-35): message to stderr, exit code 99
static void check(rt_status st, const char* what) {
    if (st == RT_OK) return;
    fprintf(stderr, "%s failed: %s -- %s\n", what, rt_strerror(st), rt_last_error_detail());
    exit(99);
}

int main(int argc, char** argv) {
    std::string scene_name = "bouncing", texture_path, aov_prefix, through_prefix;
    rt_aov_through_desc chain;   // the binding's defaults (AOV_THROUGH_DEFAULTS)
    memset(&chain, 0, sizeof(chain));
    chain.max_bounces = 8; chain.fuzz_limit = 0.0f;
    bool denoise_through = false, chain_given = false;
    int nx = 0, ny = 0, ns = 0, device = 0, gpus = 1, progressive = 0;
    bool p6 = false, adaptive = false;
    float threshold = 0.f;
    int upscale = 0;
    int min_spp = 0, denoise = 0, batches = -1;   // batches: -1 = no --denoise-variance, 0 = B left out
    int orbit_frames = 0;
    double orbit_degrees = 0.0;
    bool temporal = false, bounce = false, spin = false, follow_instances = false, grow = false, follow_quads = false;
    double bounce_height = 0.0, spin_degrees = 0.0, grow_amount = 0.0;
    std::string out_prefix;
    unsigned long long seed = 1984ull;
    for (int a = 1; a < argc; ++a) {
        std::string k = argv[a];
        auto val = [&]() -> const char* { if (a + 1 >= argc) { fprintf(stderr, "missing value for %s\n", k.c_str()); exit(2); } return argv[++a]; };
        if (k == "--scene") scene_name = val();
        else if (k == "--nx") nx = atoi(val());
        else if (k == "--ny") ny = atoi(val());
        else if (k == "--ns") ns = atoi(val());
        else if (k == "--seed") seed = strtoull(val(), nullptr, 10);
        else if (k == "--texture") texture_path = val();
        else if (k == "--device") device = atoi(val());
        else if (k == "--gpus") gpus = atoi(val());
        else if (k == "--p6") p6 = true;                        // binary PPM (clamped); the default is the reference's ASCII P3
        else if (k == "--progressive") progressive = atoi(val());   // render in windows of K samples (rt_render_window): same pixels, a frame after each
        else if (k == "--adaptive") { adaptive = true; threshold = strtof(val(), nullptr); }
        else if (k == "--min-spp") min_spp = atoi(val());
        else if (k == "--aov") aov_prefix = val();
        else if (k == "--aov-through") through_prefix = val();
        else if (k == "--through-bounces") {
            chain.max_bounces = atoi(val()); chain_given = true;
            if (chain.max_bounces < 0 || chain.max_bounces > 16) { fprintf(stderr, "--through-bounces N: N must be in 0..16\n"); return 2; }
        }
        else if (k == "--through-fuzz") {
            chain.fuzz_limit = strtof(val(), nullptr); chain_given = true;
            if (!(std::isfinite(chain.fuzz_limit) && chain.fuzz_limit >= 0.f)) { fprintf(stderr, "--through-fuzz F: F must be finite and >= 0\n"); return 2; }
        }
        else if (k == "--denoise-through") denoise_through = true;
        else if (k == "--upscale") {
            upscale = atoi(val());
            if (upscale < 2 || upscale > 8) { fprintf(stderr, "--upscale F: F must be in 2..8\n"); return 2; }
        }
        else if (k == "--denoise") {   // K is optional: the next argument when it is a number
            denoise = 5;
            if (a + 1 < argc && argv[a + 1][0] >= '0' && argv[a + 1][0] <= '9') denoise = atoi(argv[++a]);
            if (denoise < 1 || denoise > 8) { fprintf(stderr, "--denoise K: K must be in 1..8\n"); return 2; }
        }
        else if (k == "--denoise-variance") {   // B is optional, as K above
            batches = 0;
            if (a + 1 < argc && argv[a + 1][0] >= '0' && argv[a + 1][0] <= '9') {
                batches = atoi(argv[++a]);
                if (batches < 2 || batches > 64) { fprintf(stderr, "--denoise-variance B: B must be in 2..64\n"); return 2; }
            }
        }
        else if (k == "--orbit") {
            orbit_frames = atoi(val());
            orbit_degrees = strtod(val(), nullptr);
            if (orbit_frames < 1 || orbit_frames > 1000 || !std::isfinite(orbit_degrees)) { fprintf(stderr, "--orbit FRAMES DEGREES: FRAMES must be in 1..1000 and DEGREES finite\n"); return 2; }
        }
        else if (k == "--out") out_prefix = val();
        else if (k == "--temporal") temporal = true;
        else if (k == "--follow-instances") follow_instances = true;
        else if (k == "--bounce") {
            bounce = true;
            bounce_height = strtod(val(), nullptr);
            if (!std::isfinite(bounce_height) || bounce_height < 0.0) { fprintf(stderr, "--bounce HEIGHT: HEIGHT must be finite and >= 0\n"); return 2; }
        }
        else if (k == "--spin") {
            spin = true;
            spin_degrees = strtod(val(), nullptr);
            if (!std::isfinite(spin_degrees)) { fprintf(stderr, "--spin DEGREES: DEGREES must be finite\n"); return 2; }
        }
        else if (k == "--grow") {
            grow = true;
            grow_amount = strtod(val(), nullptr);
            if (!std::isfinite(grow_amount) || !(fabs(grow_amount) < 1.0)) { fprintf(stderr, "--grow AMOUNT: AMOUNT must be finite and |AMOUNT| < 1\n"); return 2; }
        }
        else if (k == "--follow-quads") follow_quads = true;
        else if (k == "--list") { int n = 0; const char* const* v = rtw::scene_names(&n); for (int i = 0; i < n; ++i) printf("%s\n", v[i]); return 0; }
        else { fprintf(stderr, "unknown argument %s\n", k.c_str()); return 2; }
    }

    if (adaptive && (progressive > 0 || gpus > 1)) { fprintf(stderr, "--adaptive cannot be combined with --progressive or --gpus > 1\n"); return 2; }
    if (!aov_prefix.empty() && gpus > 1) { fprintf(stderr, "--aov cannot be combined with --gpus > 1\n"); return 2; }
    if (!through_prefix.empty() && gpus > 1) { fprintf(stderr, "--aov-through cannot be combined with --gpus > 1\n"); return 2; }
    if (denoise_through && !denoise) { fprintf(stderr, "--denoise-through needs --denoise\n"); return 2; }
    if (chain_given && through_prefix.empty() && !denoise_through) { fprintf(stderr, "--through-bounces and --through-fuzz need --aov-through or --denoise-through\n"); return 2; }
    if (denoise && (progressive > 0 || gpus > 1)) { fprintf(stderr, "--denoise cannot be combined with --progressive or --gpus > 1\n"); return 2; }
    if (batches >= 0 && !denoise) { fprintf(stderr, "--denoise-variance needs --denoise\n"); return 2; }
    if (batches >= 0 && adaptive) { fprintf(stderr, "--denoise-variance cannot be combined with --adaptive\n"); return 2; }
    if (min_spp > 0 && !adaptive) { fprintf(stderr, "--min-spp needs --adaptive\n"); return 2; }
    if (orbit_frames > 0 && out_prefix.empty()) { fprintf(stderr, "--orbit needs --out PREFIX\n"); return 2; }
    if (orbit_frames == 0 && (temporal || !out_prefix.empty())) { fprintf(stderr, "--temporal and --out need --orbit\n"); return 2; }
    if (orbit_frames == 0 && bounce) { fprintf(stderr, "--bounce needs --orbit\n"); return 2; }
    if (orbit_frames == 0 && spin) { fprintf(stderr, "--spin needs --orbit\n"); return 2; }
    if (spin && temporal) { fprintf(stderr, "--spin cannot be combined with --temporal: the reprojection does not follow a moved instance\n"); return 2; }
    if (follow_instances && !spin) { fprintf(stderr, "--follow-instances needs --orbit FRAMES DEGREES --spin DEGREES: it accumulates the frames and follows the instances --spin turns\n"); return 2; }
    if (orbit_frames == 0 && grow) { fprintf(stderr, "--grow needs --orbit\n"); return 2; }
    if (grow && temporal) { fprintf(stderr, "--grow cannot be combined with --temporal: the plain accumulation does not follow a box that changes size (--follow-quads does)\n"); return 2; }
    if (follow_quads && !grow) { fprintf(stderr, "--follow-quads needs --orbit FRAMES DEGREES --grow AMOUNT: it accumulates the frames and follows the faces of the boxes --grow resizes\n"); return 2; }
    if (orbit_frames > 0 && (gpus > 1 || progressive > 0 || adaptive || denoise || !aov_prefix.empty() || !through_prefix.empty())) {
        fprintf(stderr, "--orbit cannot be combined with --gpus > 1, --progressive, --adaptive, --denoise, --aov or --aov-through\n");
        return 2;
    }

    if (upscale && (gpus > 1 || progressive > 0 || adaptive || orbit_frames > 0 || !aov_prefix.empty() || !through_prefix.empty() || batches >= 0 || denoise_through)) {
        fprintf(stderr, "--upscale cannot be combined with --gpus > 1, --progressive, --adaptive, --orbit, --aov, --aov-through, --denoise-variance or --denoise-through\n");
        return 2;
    }

    std::vector<unsigned char> tex;
    int tw = 0, th = 0;
    if (!texture_path.empty() && !rtw::load_ppm(texture_path, tex, tw, th)) {
        fprintf(stderr, "could not read texture '%s' (binary or ASCII PPM expected)\n", texture_path.c_str());
        return 1;   // the reference returns 1 when its texture fails to load (main.cu:817-820)
    }
    std::string err;
    auto scene = rtw::build_scene(scene_name, nx, ny, tex.empty() ? nullptr : tex.data(), tw, th, err);
    if (!scene) { fprintf(stderr, "%s\n", err.c_str()); return 2; }
    if (ns > 0) scene->ns = ns;
    if (upscale && (scene->nx % upscale || scene->ny % upscale)) {
        fprintf(stderr, "--upscale %d: the image size %dx%d is not a multiple of it\n", upscale, scene->nx, scene->ny);
        return 2;
    }
    if (batches == 0) {   // the largest divisor of ns that is at most 16
        batches = scene->ns < 16 ? scene->ns : 16;
        while (batches > 1 && scene->ns % batches) --batches;
    }
    if (batches == 1) { fprintf(stderr, "--denoise-variance: --ns %d has no divisor in 2..16; give B (2..64, a divisor of --ns)\n", scene->ns); return 2; }
    if (batches >= 0 && scene->ns % batches) {
        fprintf(stderr, "--denoise-variance: --ns %d is not a multiple of B = %d\n", scene->ns, batches);
        return 2;
    }

    rtw::flat_scene flat;
    rt_status st = rtw::flatten(scene->world, *scene->cam, flat, err, scene->created.data(), (int)scene->created.size());
    if (st != RT_OK) { fprintf(stderr, "flatten: %s\n", err.c_str()); return 2; }
    const rt_scene_desc desc = flat.desc();
    if (bounce && !flat.instances.empty()) {
        fprintf(stderr, "--bounce: scene '%s' has instances, and a sphere under an instance cannot move (rt_scene_update_spheres)\n", scene_name.c_str());
        return 2;
    }
    if (spin) {
        bool rotated = false;
        for (const rt_instance& in : flat.instances) rotated = rotated || (in.flags & RT_INST_ROTATE_Y);
        if (!rotated) { fprintf(stderr, "--spin: scene '%s' has no rotated instance\n", scene_name.c_str()); return 2; }
    }

    if (grow && flat.boxes.empty()) { fprintf(stderr, "--grow: scene '%s' has no box\n", scene_name.c_str()); return 2; }

    fprintf(stderr, "Rendering a %dx%d image in 8x8 blocks.\n", scene->nx, scene->ny);
    rt_frame_desc f;
    memset(&f, 0, sizeof(f));
    f.nx = scene->nx; f.ny = scene->ny; f.ns = scene->ns; f.gamma = scene->gamma;
    f.background[0] = scene->background.x(); f.background[1] = scene->background.y(); f.background[2] = scene->background.z();
    f.use_gradient_bg = scene->use_gradient_bg;
    f.seed_base = seed;
    f.tile_rows = scene->ny; f.tile_first = 0; f.tile_stride = 1;
    if (denoise) f.gamma = 1.0f;   // the filter works on the linear frame; the gamma is applied after it, below

    std::vector<float> fb((size_t)scene->nx * scene->ny * 3), variance;
    rt_stats stats;
    rt_scene* dev_scene = nullptr;
    rt_multi* multi = nullptr;
    if (orbit_frames > 0) {
        // a turntable of one device scene: a camera per frame (rt_scene_set_camera), optionally accumulated over time (rt_reproject)
        const size_t px = (size_t)scene->nx * scene->ny;
        check(rt_init(device), "rt_init");
        check(rt_scene_create(&desc, &dev_scene), "rt_scene_create");
        const rtw::camera& c0 = *scene->cam;
        const bool accumulate = temporal || follow_instances || follow_quads, keep_inst = follow_instances || follow_quads;
        if (accumulate) f.gamma = 1.0f;
        struct features { std::vector<float> normal, depth, alpha; std::vector<int32_t> prim, inst; };
        features feat[2];
        for (features& x : feat) { x.normal.resize(px * 3); x.depth.resize(px); x.alpha.resize(px); x.prim.resize(px); if (keep_inst) x.inst.resize(px); }
        std::vector<float> acc[2] = {std::vector<float>(px * 3), std::vector<float>(px * 3)}, len[2] = {std::vector<float>(px), std::vector<float>(px)};
        rt_camera prev_cam;
        memset(&prev_cam, 0, sizeof(prev_cam));
        std::vector<rt_sphere> records[2] = {flat.spheres, flat.spheres};   // --bounce: the records of this frame and of the previous one
        std::vector<rt_instance> inst_records[2] = {flat.instances, flat.instances};   // --follow-instances: likewise, as the scene holds them
        std::vector<rt_quad> quad_records[2] = {flat.quads, flat.quads};   // --follow-quads: likewise
        double ms = 0.0;
        for (int k = 0; k < orbit_frames; ++k) {
            if (grow) {
                std::vector<rt_quad> now = flat.quads;
                for (const rt_box& box : flat.boxes) {
                    const rt_quad* face = &flat.quads[(size_t)box.first_quad];
                    float lo[3], hi[3];
                    for (int c = 0; c < 3; ++c) { lo[c] = INFINITY; hi[c] = -INFINITY; }
                    for (int fc = 0; fc < 6; ++fc)
                        for (int c = 0; c < 3; ++c) {
                            const float qu = face[fc].Q[c] + face[fc].u[c];
                            const float corner[4] = {face[fc].Q[c], qu, face[fc].Q[c] + face[fc].v[c], qu + face[fc].v[c]};
                            for (float x : corner) { lo[c] = fminf(lo[c], x); hi[c] = fmaxf(hi[c], x); }
                        }
                    hi[1] = (float)((double)lo[1] + ((double)hi[1] - (double)lo[1]) * (1.0 + grow_amount * sin(2.0 * 3.14159265358979323846 * (double)k / (double)orbit_frames)));
                    if (rtw_box_records(lo, hi, face[0].mat, &now[(size_t)box.first_quad]) != 0) { fprintf(stderr, "--grow: make_box failed\n"); return 1; }
                }
                rt_quad_update up;
                memset(&up, 0, sizeof(up));
                up.count = (int32_t)now.size(); up.first = 0; up.quads = now.data();
                check(rt_scene_update_quads(dev_scene, &up, /*quads_on_device=*/0, /*recalibrate=*/0, /*stream=*/nullptr), "rt_scene_update_quads");
                if (follow_quads) check(rt_scene_get_quads(dev_scene, quad_records[k & 1].data(), (int32_t)quad_records[k & 1].size()), "rt_scene_get_quads");
            }
            if (bounce && !flat.spheres.empty()) {
                std::vector<rt_sphere>& now = records[k & 1];
                for (size_t i = 0; i < now.size(); ++i) {
                    const rt_sphere& base = flat.spheres[i];
                    if (!(base.radius > 0.f && base.radius < 0.5f)) continue;
                    now[i].c0[1] = (float)((double)base.c0[1] + bounce_height * fabs(sin(3.14159265358979323846 * ((double)k / orbit_frames + 0.61803398875 * (double)i))));
                }
                rt_sphere_update up;
                memset(&up, 0, sizeof(up));
                up.count = (int32_t)now.size(); up.first = 0; up.spheres = now.data();
                check(rt_scene_update_spheres(dev_scene, &up, /*spheres_on_device=*/0, /*recalibrate=*/0, /*stream=*/nullptr), "rt_scene_update_spheres");
            }
            if (spin) {
                std::vector<rt_instance> now = flat.instances;
                for (rt_instance& in : now) {
                    if (!(in.flags & RT_INST_ROTATE_Y)) continue;
                    const double a = atan2((double)in.sin_t, (double)in.cos_t) + (double)k * spin_degrees * 3.14159265358979323846 / 180.0;
                    in.sin_t = (float)sin(a); in.cos_t = (float)cos(a);
                }
                rt_instance_update up;
                memset(&up, 0, sizeof(up));
                up.count = (int32_t)now.size(); up.first = 0; up.instances = now.data();
                check(rt_scene_update_instances(dev_scene, &up, /*instances_on_device=*/0, /*recalibrate=*/0, /*stream=*/nullptr), "rt_scene_update_instances");
                if (keep_inst) check(rt_scene_get_instances(dev_scene, inst_records[k & 1].data(), (int32_t)inst_records[k & 1].size()), "rt_scene_get_instances");
            }
            const double th = (double)k * orbit_degrees / (double)orbit_frames * 3.14159265358979323846 / 180.0;
            const double dx = (double)c0.lookfrom.x() - c0.lookat.x(), dz = (double)c0.lookfrom.z() - c0.lookat.z();
            const rtw::vec3 eye((float)(c0.lookat.x() + cos(th) * dx + sin(th) * dz), c0.lookfrom.y(), (float)(c0.lookat.z() - sin(th) * dx + cos(th) * dz));
            const rt_camera cam = rtw::camera_desc(rtw::camera(eye, c0.lookat, c0.vup, c0.vfov, c0.aspect, c0.aperture, c0.focus_dist, c0.time0, c0.time1));
            check(rt_scene_set_camera(dev_scene, &cam, /*recalibrate=*/0), "rt_scene_set_camera");
            check(rt_render(dev_scene, &f, fb.data(), /*fb_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1, &stats), "rt_render");
            ms += stats.ms_render;
            if (accumulate) {
                features& cur = feat[k & 1];
                const features& old = feat[(k + 1) & 1];
                rt_frame_desc ff = f;
                if (ff.ns > 16) ff.ns = 16;
                rt_aov_desc aov;
                memset(&aov, 0, sizeof(aov));
                aov.normal = cur.normal.data(); aov.depth = cur.depth.data(); aov.alpha = cur.alpha.data(); aov.prim = cur.prim.data();
                if (keep_inst) aov.inst = cur.inst.data();
                check(rt_render_aov(dev_scene, &ff, &aov, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_render_aov");
                rt_reproject_desc rd;
                memset(&rd, 0, sizeof(rd));
                rd.nx = scene->nx; rd.ny = scene->ny; rd.cur = cam; rd.prev = k ? prev_cam : cam;
                rd.color = fb.data(); rd.depth = cur.depth.data(); rd.alpha = cur.alpha.data();
                if (k) {
                    rd.normal = cur.normal.data(); rd.prim = cur.prim.data();
                    rd.history = acc[(k + 1) & 1].data(); rd.history_len = len[(k + 1) & 1].data();
                    rd.prev_depth = old.depth.data(); rd.prev_alpha = old.alpha.data(); rd.prev_normal = old.normal.data(); rd.prev_prim = old.prim.data();
                }
                rd.out = acc[k & 1].data(); rd.out_len = len[k & 1].data();
                rd.alpha_min = 0.5f; rd.depth_tol = 0.05f; rd.normal_min = 0.5f; rd.max_history = 32.0f;   // the binding's REPROJECT_DEFAULTS
                if (follow_quads && k) {   // the history follows the faces that moved since the previous frame, and whatever else did
                    rt_reproject_motion_desc md;
                    memset(&md, 0, sizeof(md));
                    if (bounce) {
                        md.n_spheres = (int32_t)flat.spheres.size();
                        md.spheres = md.n_spheres ? records[k & 1].data() : nullptr; md.prev_spheres = md.n_spheres ? records[(k + 1) & 1].data() : nullptr;
                    }
                    md.n_media = (int32_t)flat.media.size();
                    md.media = md.n_media ? flat.media.data() : nullptr;
                    md.time = (float)(0.5 * (cam.time0 + cam.time1)); md.prev_time = (float)(0.5 * (prev_cam.time0 + prev_cam.time1));
                    rt_reproject_instance_desc id;
                    memset(&id, 0, sizeof(id));
                    id.n_instances = (int32_t)flat.instances.size();
                    id.instances = id.n_instances ? inst_records[k & 1].data() : nullptr; id.prev_instances = id.n_instances ? inst_records[(k + 1) & 1].data() : nullptr;
                    id.inst = cur.inst.data(); id.prev_inst = old.inst.data();
                    rt_reproject_quad_desc qd;
                    memset(&qd, 0, sizeof(qd));
                    qd.n_quads = (int32_t)flat.quads.size();
                    qd.quads = quad_records[k & 1].data(); qd.prev_quads = quad_records[(k + 1) & 1].data();
                    check(rt_reproject_quads(&rd, &md, &id, &qd, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_reproject_quads");
                } else if (bounce && k) {   // the history follows the spheres that moved since the previous frame
                    rt_reproject_motion_desc md;
                    memset(&md, 0, sizeof(md));
                    md.n_spheres = (int32_t)flat.spheres.size(); md.n_media = (int32_t)flat.media.size();
                    md.spheres = md.n_spheres ? records[k & 1].data() : nullptr; md.prev_spheres = md.n_spheres ? records[(k + 1) & 1].data() : nullptr;
                    md.media = md.n_media ? flat.media.data() : nullptr;
                    md.time = (float)(0.5 * (cam.time0 + cam.time1)); md.prev_time = (float)(0.5 * (prev_cam.time0 + prev_cam.time1));   // the binding's default
                    check(rt_reproject_moving(&rd, &md, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_reproject_moving");
                } else if (follow_instances && k) {   // ... the instances that turned
                    rt_reproject_motion_desc md;
                    memset(&md, 0, sizeof(md));
                    md.n_media = (int32_t)flat.media.size();
                    md.media = md.n_media ? flat.media.data() : nullptr;
                    md.time = (float)(0.5 * (cam.time0 + cam.time1)); md.prev_time = (float)(0.5 * (prev_cam.time0 + prev_cam.time1));
                    rt_reproject_instance_desc id;
                    memset(&id, 0, sizeof(id));
                    id.n_instances = (int32_t)flat.instances.size();
                    id.instances = inst_records[k & 1].data(); id.prev_instances = inst_records[(k + 1) & 1].data();
                    id.inst = cur.inst.data(); id.prev_inst = old.inst.data();
                    check(rt_reproject_instances(&rd, &md, &id, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_reproject_instances");
                } else {
                    check(rt_reproject(&rd, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_reproject");
                }
                prev_cam = cam;
                fb = acc[k & 1];
                if (scene->gamma != 1.0f) for (float& c : fb) c = powf(c, 1.0f / scene->gamma);
            }
            char name[32];
            snprintf(name, sizeof(name), "_%03d.ppm", k);
            const std::string path = out_prefix + name;
            FILE* out = fopen(path.c_str(), "wb");
            if (!out) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
            if (p6) rtw::write_ppm_p6(out, fb.data(), scene->nx, scene->ny, scene->ppm_double_scale);
            else rtw::write_ppm_p3(out, fb.data(), scene->nx, scene->ny, scene->ppm_double_scale);
            fclose(out);
            fprintf(stderr, "frame %d: %.3f ms -> %s\n", k, stats.ms_render, path.c_str());
        }
        fprintf(stderr, "took %g seconds.\n", ms * 1e-3);
        check(rt_scene_destroy(dev_scene), "rt_scene_destroy");
        check(rt_shutdown(), "rt_shutdown");
        return 0;
    }
    if (upscale) {
        // paths on the coarse grid, guides on both, rt_upscale (DeviceScene.render_upscaled of the binding, call for call)
        const int lx = scene->nx / upscale, ly = scene->ny / upscale;
        const size_t px = (size_t)scene->nx * scene->ny, px_lo = (size_t)lx * ly;
        check(rt_init(device), "rt_init");
        check(rt_scene_create(&desc, &dev_scene), "rt_scene_create");
        rt_frame_desc lo = f;
        lo.nx = lx; lo.ny = ly; lo.gamma = 1.0f; lo.tile_rows = ly;
        std::vector<float> low(px_lo * 3), albedo_lo(px_lo * 3), normal_lo(px_lo * 3), depth_lo(px_lo), albedo(px * 3), normal(px * 3), depth(px);
        check(rt_render(dev_scene, &lo, low.data(), /*fb_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1, &stats), "rt_render");
        fprintf(stderr, "took %g seconds.\n", stats.ms_render * 1e-3);
        if (lo.ns > 16) lo.ns = 16;
        rt_aov_desc aov;
        memset(&aov, 0, sizeof(aov));
        aov.albedo = albedo_lo.data(); aov.normal = normal_lo.data(); aov.depth = depth_lo.data();
        check(rt_render_aov(dev_scene, &lo, &aov, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_render_aov");
        if (denoise) {
            rt_denoise_desc dn;
            memset(&dn, 0, sizeof(dn));
            dn.nx = lx; dn.ny = ly;
            dn.color = low.data(); dn.albedo = albedo_lo.data(); dn.normal = normal_lo.data(); dn.depth = depth_lo.data();
            dn.out = low.data();
            dn.iterations = denoise; dn.normal_sharpness = 4; dn.demodulate = 1;
            dn.sigma_color = 2.0f; dn.color_floor = 0.01f; dn.sigma_depth = 0.2f;
            check(rt_denoise(&dn, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_denoise");
        }
        rt_frame_desc full = f;
        full.gamma = 1.0f;
        if (full.ns > 16) full.ns = 16;
        aov.albedo = albedo.data(); aov.normal = normal.data(); aov.depth = depth.data();
        check(rt_render_aov(dev_scene, &full, &aov, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_render_aov");
        rt_upscale_desc u;
        memset(&u, 0, sizeof(u));
        u.nx = scene->nx; u.ny = scene->ny; u.factor = upscale;
        u.normal_sharpness = 4; u.demodulate = 1; u.sigma_depth = 0.2f; u.min_weight = 0.015625f;
        u.color_lo = low.data(); u.albedo_lo = albedo_lo.data(); u.normal_lo = normal_lo.data(); u.depth_lo = depth_lo.data();
        u.albedo = albedo.data(); u.normal = normal.data(); u.depth = depth.data();
        u.out = fb.data();
        check(rt_upscale(&u, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_upscale");
        if (scene->gamma != 1.0f) for (float& c : fb) c = powf(c, 1.0f / scene->gamma);
        if (p6) rtw::write_ppm_p6(stdout, fb.data(), scene->nx, scene->ny, scene->ppm_double_scale);
        else rtw::write_ppm_p3(stdout, fb.data(), scene->nx, scene->ny, scene->ppm_double_scale);
        check(rt_scene_destroy(dev_scene), "rt_scene_destroy");
        check(rt_shutdown(), "rt_shutdown");
        return 0;
    }
    if (gpus > 1) {
        check(rt_init_devices(gpus), "rt_init_devices");
        check(rt_multi_create(&desc, gpus, &multi), "rt_multi_create");
        check(rt_multi_render(multi, &f, fb.data(), /*fb_on_device=*/0, /*tile_rows=*/4, &stats), "rt_multi_render");
    } else {
        check(rt_init(device), "rt_init");
        check(rt_scene_create(&desc, &dev_scene), "rt_scene_create");
        if (adaptive) {
            rt_adaptive_desc ad;
            ad.max_spp = scene->ns;
            if (min_spp <= 0) {   // the smallest checkpoint of max_spp that is even and >= 16 (max_spp itself below that)
                min_spp = scene->ns;
                while (min_spp % 4 == 0 && min_spp / 2 >= 16) min_spp /= 2;
            }
            ad.min_spp = min_spp; ad.threshold = threshold; ad.floor = 0.01f;
            check(rt_render_adaptive(dev_scene, &f, &ad, fb.data(), /*fb_on_device=*/0, /*spp_out=*/nullptr, /*stream=*/nullptr, &stats),
                  "rt_render_adaptive");
            fprintf(stderr, "adaptive: spp %d..%d, mean %.2f, %d passes\n", ad.min_spp, ad.max_spp,
                    (double)stats.samples / ((double)scene->nx * scene->ny), stats.reserved);
        } else if (progressive > 0) {
            // progressive accumulation: the per-pixel XORWOW state and colour sum are carried from window to window (the
            // reference writes its curandState back for exactly this, main.cu:126); the last window's frame is the one-shot frame
            void* state = nullptr;
            check(rt_progressive_state_create(dev_scene, &f, &state), "rt_progressive_state_create");
            rt_stats part;
            memset(&stats, 0, sizeof(stats));
            for (int begin = 0; begin < scene->ns; begin += progressive) {
                const int end = begin + progressive < scene->ns ? begin + progressive : scene->ns;
                check(rt_render_window(dev_scene, &f, fb.data(), 0, state, begin, end, nullptr, 1, &part), "rt_render_window");
                stats.rays += part.rays; stats.ms_render += part.ms_render;
                fprintf(stderr, "samples [%d, %d): %.3f ms\n", begin, end, part.ms_render);
            }
            check(rt_progressive_state_destroy(dev_scene, state), "rt_progressive_state_destroy");
        } else if (batches >= 2) {
            rt_variance_desc vd;
            vd.batches = batches; vd.reserved = 0;
            variance.resize((size_t)scene->nx * scene->ny);
            check(rt_render_variance(dev_scene, &f, &vd, fb.data(), /*fb_on_device=*/0, variance.data(), /*stream=*/nullptr, &stats), "rt_render_variance");
        } else {
            check(rt_render(dev_scene, &f, fb.data(), /*fb_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1, &stats), "rt_render");
        }
    }
    fprintf(stderr, "took %g seconds.\n", stats.ms_render * 1e-3);
    fprintf(stderr, "{\"scene\": \"%s\", \"nx\": %d, \"ny\": %d, \"ns\": %d, \"gpus\": %d, \"rays\": %llu, \"ms_render\": %.3f, \"mrays_per_s\": %.1f}\n",
            scene_name.c_str(), scene->nx, scene->ny, scene->ns, gpus, (unsigned long long)stats.rays, stats.ms_render,
            stats.ms_render > 0 ? (double)stats.rays / (stats.ms_render * 1e3) : 0.0);

    if (denoise) {
        const size_t px = (size_t)scene->nx * scene->ny;
        auto apply_gamma = [&](std::vector<float>& img) {
            if (scene->gamma != 1.0f) for (float& c : img) c = powf(c, 1.0f / scene->gamma);
        };
        std::vector<float> albedo(px * 3), normal(px * 3), depth(px);
        rt_frame_desc ff = f;
        if (ff.ns > 16) ff.ns = 16;
        rt_aov_desc aov;
        memset(&aov, 0, sizeof(aov));
        aov.albedo = albedo.data(); aov.normal = normal.data(); aov.depth = depth.data();
        if (denoise_through) check(rt_render_aov_through(dev_scene, &ff, &aov, &chain, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_render_aov_through");
        else check(rt_render_aov(dev_scene, &ff, &aov, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_render_aov");
        if (!aov_prefix.empty()) {
            std::vector<float> noisy = fb;
            apply_gamma(noisy);
            const std::string path = aov_prefix + "_noisy.ppm";
            FILE* out = fopen(path.c_str(), "wb");
            if (!out) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
            if (p6) rtw::write_ppm_p6(out, noisy.data(), scene->nx, scene->ny, scene->ppm_double_scale);
            else rtw::write_ppm_p3(out, noisy.data(), scene->nx, scene->ny, scene->ppm_double_scale);
            fclose(out);
        }
        rt_denoise_desc dn;
        memset(&dn, 0, sizeof(dn));
        dn.nx = scene->nx; dn.ny = scene->ny;
        dn.color = fb.data(); dn.albedo = albedo.data(); dn.normal = normal.data(); dn.depth = depth.data();
        dn.out = fb.data();
        dn.iterations = denoise; dn.normal_sharpness = 4; dn.demodulate = 1;
        dn.sigma_color = 2.0f; dn.color_floor = 0.01f; dn.sigma_depth = 0.2f;
        if (batches >= 2) {
            rt_denoise_variance_desc dv;
            memset(&dv, 0, sizeof(dv));
            dv.variance = variance.data();
            dv.sigma_variance = 3.0f; dv.variance_floor = 1e-4f;
            dn.sigma_color = 0.0f;
            check(rt_denoise_variance(&dn, &dv, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_denoise_variance");
        } else {
            check(rt_denoise(&dn, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_denoise");
        }
        apply_gamma(fb);
    }

    if (p6) rtw::write_ppm_p6(stdout, fb.data(), scene->nx, scene->ny, scene->ppm_double_scale);
    else rtw::write_ppm_p3(stdout, fb.data(), scene->nx, scene->ny, scene->ppm_double_scale);

    // the feature buffers of the frame as images: rt_render_aov's, or with `through` rt_render_aov_through's and its share buffer
    auto write_features = [&](const std::string& prefix, bool through) -> bool {
        const size_t px = (size_t)scene->nx * scene->ny;
        std::vector<float> albedo(px * 3), normal(px * 3), depth(px), grey(px * 3), share(through ? px : 0), share3(through ? px * 3 : 0);
        rt_aov_desc aov;
        memset(&aov, 0, sizeof(aov));
        aov.albedo = albedo.data(); aov.normal = normal.data(); aov.depth = depth.data();
        if (through) {
            rt_aov_through_desc t = chain;
            t.through = share.data();
            check(rt_render_aov_through(dev_scene, &f, &aov, &t, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_render_aov_through");
            for (size_t p = 0; p < px; ++p) share3[3 * p] = share3[3 * p + 1] = share3[3 * p + 2] = share[p];
        } else {
            check(rt_render_aov(dev_scene, &f, &aov, /*buffers_on_device=*/0, /*stream=*/nullptr, /*blocking=*/1), "rt_render_aov");
        }
        for (float& c : normal) c = 0.5f * c + 0.5f;
        float t_far = 0.f;
        for (float t : depth) if (t > t_far) t_far = t;
        for (size_t p = 0; p < px; ++p) grey[3 * p] = grey[3 * p + 1] = grey[3 * p + 2] = t_far > 0.f ? depth[p] / t_far : 0.f;
        const struct { const char* name; const float* data; } files[] = {{"albedo", albedo.data()}, {"normal", normal.data()}, {"depth", grey.data()},
                                                                         {"through", share3.data()}};
        for (const auto& o : files) {
            if (!through && o.data == share3.data()) continue;
            const std::string path = prefix + "." + o.name + ".ppm";
            FILE* out = fopen(path.c_str(), "wb");
            if (!out) { fprintf(stderr, "cannot write %s\n", path.c_str()); return false; }
            if (p6) rtw::write_ppm_p6(out, o.data, scene->nx, scene->ny, false);
            else rtw::write_ppm_p3(out, o.data, scene->nx, scene->ny, false);
            fclose(out);
        }
        return true;
    };
    if (!aov_prefix.empty() && !write_features(aov_prefix, false)) return 1;
    if (!through_prefix.empty() && !write_features(through_prefix, true)) return 1;

    if (multi) check(rt_multi_destroy(multi), "rt_multi_destroy");
    if (dev_scene) check(rt_scene_destroy(dev_scene), "rt_scene_destroy");
    check(rt_shutdown(), "rt_shutdown");
    return 0;
}
