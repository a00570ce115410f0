// rt_multi.hip -- several GPUs of one node behind the C ABI (include/rt_abi.h, rt_multi_*): one host thread, one
// scene replica and one stream per device, the frame cut into interleaved row tiles, one RCCL gather
// of the compact per-device row buffers to device 0 over xGMI, and a small kernel that puts the rows back into the
// reference's frame layout (pixel_index = j*nx + i, row 0 = bottom, main.cu:115).  No ray crosses a device and the
// per-pixel seed is seed_base + GLOBAL pixel index, so the frame is bit-identical to the one-GPU frame.
//
// RCCL is loaded with dlopen, and only when a gather is needed (n_gpus > 1, or the "multi_force_rccl" option on a
// one-GPU box): a process that also runs PyTorch (bench.py) already carries torch's own copy of the library, and
// resolving ncclGather through the global symbol table would mix the two.
#include <dlfcn.h>

#include <chrono>

#include "rt_host.h"

using namespace rt_host;

namespace {

// a failed call's status, with the error state this file's entries leave: the HIP or RCCL code (0: none) and the text
rt_status fail(rt_status st, int code, const std::string& detail) { g_last_hip_error = code; g_detail = detail; return st; }

// the handful of RCCL entry points used, with the types of <rccl/rccl.h> (ncclComm_t is an opaque pointer,
// ncclFloat = 7, ncclSuccess = 0; rccl.h:36,466,52)
typedef void* nccl_comm;
typedef int (*fn_CommInitAll)(nccl_comm*, int, const int*);
typedef int (*fn_CommDestroy)(nccl_comm);
typedef int (*fn_GroupStart)();
typedef int (*fn_GroupEnd)();
typedef int (*fn_Gather)(const void*, void*, size_t, int, int, nccl_comm, hipStream_t);   // rccl.h:745
typedef const char* (*fn_GetErrorString)(int);
enum { NCCL_FLOAT = 7 };

struct rccl_api {
    void* handle = nullptr;
    fn_CommInitAll CommInitAll = nullptr;
    fn_CommDestroy CommDestroy = nullptr;
    fn_GroupStart GroupStart = nullptr;
    fn_GroupEnd GroupEnd = nullptr;
    fn_Gather Gather = nullptr;
    fn_GetErrorString GetErrorString = nullptr;
};

// `only` (tests): try exactly this name instead of the usual ones
bool load_rccl(rccl_api& r, std::string& why, const char* only = nullptr) {
    if (r.handle) return true;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    std::string last;
    for (const char* n : names) {
        if (only) n = only;
        r.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (r.handle) break;
        const char* e = dlerror();   // (returns the message once and clears it)
        last = e ? e : "?";
        if (only) break;
    }
    if (!r.handle) { why = std::string("cannot load librccl.so: ") + last; return false; }
    r.CommInitAll = (fn_CommInitAll)dlsym(r.handle, "ncclCommInitAll");
    r.CommDestroy = (fn_CommDestroy)dlsym(r.handle, "ncclCommDestroy");
    r.GroupStart = (fn_GroupStart)dlsym(r.handle, "ncclGroupStart");
    r.GroupEnd = (fn_GroupEnd)dlsym(r.handle, "ncclGroupEnd");
    r.Gather = (fn_Gather)dlsym(r.handle, "ncclGather");
    r.GetErrorString = (fn_GetErrorString)dlsym(r.handle, "ncclGetErrorString");
    if (!r.CommInitAll || !r.CommDestroy || !r.GroupStart || !r.GroupEnd || !r.Gather) {
        why = "librccl.so lacks ncclCommInitAll / ncclGather";
        dlclose(r.handle); r.handle = nullptr;
        return false;
    }
    return true;
}

// which device renders global row j, and where in that device's compact buffer (the inverse of rt_local_to_global_row)
__host__ __device__ inline void row_owner(int j, int tile_rows, int world, int& rank, int& local_row) {
    const int tile = j / tile_rows;
    rank = tile % world;
    local_row = (tile / world) * tile_rows + (j - tile * tile_rows);
}

// staging[rank][local_row][nx*3] -> frame[global_row][nx*3]; one thread per float (a row is nx*3 floats)
__global__ void rt_uninterleave_kernel(const float* staging, float* frame, int nx3, int ny, int tile_rows, int world, int max_rows) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long total = (long long)ny * nx3;
    if (idx >= total) return;
    const int j = (int)(idx / nx3), k = (int)(idx - (long long)j * nx3);
    int rank, local_row;
    row_owner(j, tile_rows, world, rank, local_row);
    frame[idx] = staging[((size_t)rank * max_rows + local_row) * nx3 + k];
}

}  // namespace

struct rt_multi {
    int n = 0;
    std::vector<rt_scene*> scenes;
    std::vector<hipStream_t> streams;
    std::vector<float*> d_local;        // per device: compact rows of this device, max_rows * nx * 3 floats
    float* d_staging = nullptr;         // device 0: the gather's receive buffer, n * max_rows * nx * 3
    float* d_frame = nullptr;           // device 0: the assembled frame
    size_t local_floats = 0, frame_floats = 0, staging_floats = 0;   // capacities of d_local[*], d_frame, d_staging
    rccl_api rccl;
    std::vector<nccl_comm> comms;
    bool comms_ready = false;
};

extern "C" {

rt_status rt_init_devices(int n_gpus) {
    if (n_gpus < 1) return fail(RT_ERR_INVALID, 0, "rt_init_devices: n_gpus must be >= 1");
    for (int d = n_gpus - 1; d >= 0; --d) {   // device 0 last: it stays the device new single-GPU scenes are created on
        const rt_status st = rt_internal_init_device(d);
        if (st != RT_OK) return st;
    }
    return RT_OK;
}

rt_status rt_multi_destroy(rt_multi* m) {
    if (!m) return RT_OK;
    for (int d = 0; d < (int)m->scenes.size(); ++d) {
        if (hipSetDevice(d) != hipSuccess) continue;
        if (d < (int)m->comms.size() && m->comms_ready && m->comms[d]) (void)m->rccl.CommDestroy(m->comms[d]);
        if (d < (int)m->d_local.size() && m->d_local[d]) (void)hipFree(m->d_local[d]);
        if (d < (int)m->streams.size() && m->streams[d]) (void)hipStreamDestroy(m->streams[d]);
        if (m->scenes[d]) (void)rt_scene_destroy(m->scenes[d]);
    }
    if (hipSetDevice(0) == hipSuccess) {
        if (m->d_staging) (void)hipFree(m->d_staging);
        if (m->d_frame) (void)hipFree(m->d_frame);
    }
    if (m->rccl.handle) dlclose(m->rccl.handle);
    delete m;
    return RT_OK;
}

rt_status rt_multi_create(const rt_scene_desc* desc, int n_gpus, rt_multi** out) {
    if (!out) return fail(RT_ERR_INVALID, 0, "null output pointer");
    *out = nullptr;
    if (n_gpus < 1 || n_gpus > 16) return fail(RT_ERR_INVALID, 0, "rt_multi_create: n_gpus must be 1..16");
    rt_multi* m = new rt_multi;
    m->n = n_gpus;
    m->scenes.assign((size_t)n_gpus, nullptr);
    m->streams.assign((size_t)n_gpus, nullptr);
    m->d_local.assign((size_t)n_gpus, nullptr);
    for (int d = 0; d < n_gpus; ++d) {
        const rt_status st = rt_internal_scene_create_on(d, desc, &m->scenes[d]);   // also makes device d current
        if (st != RT_OK) { rt_multi_destroy(m); return st; }
        hipError_t e = hipStreamCreateWithFlags(&m->streams[d], hipStreamNonBlocking);
        if (e != hipSuccess) { rt_multi_destroy(m); return fail(RT_ERR_HIP, (int)e, "rt_multi_create: hipStreamCreate failed"); }
    }
    *out = m;
    return RT_OK;
}

int32_t rt_multi_device_count(const rt_multi* m) { return m ? m->n : 0; }

// One call on every replica; device 0 last, so that it stays the current device.  The call's checks run in the first of these
// calls, before any HIP call, and a refusal there leaves every replica untouched.
extern "C++" template <class Call>
static rt_status on_every_replica(rt_multi* m, const char* null_handle, Call&& call) {
    if (!m) return fail(RT_ERR_INVALID, 0, null_handle);
    for (int d = m->n - 1; d >= 0; --d) {
        const rt_status st = call(m->scenes[d]);
        if (st != RT_OK) return st;
    }
    return RT_OK;
}

rt_status rt_multi_set_camera(rt_multi* m, const rt_camera* camera, int recalibrate) {
    return on_every_replica(m, "rt_multi_set_camera: null rt_multi", [&](rt_scene* s) { return rt_scene_set_camera(s, camera, recalibrate); });
}

// rt_scene_update_spheres, _instances, _quads with host records on every replica; each replica's default stream
rt_status rt_multi_update_spheres(rt_multi* m, const rt_sphere_update* update, int recalibrate) {
    return on_every_replica(m, "rt_multi_update_spheres: null rt_multi", [&](rt_scene* s) { return rt_scene_update_spheres(s, update, 0, recalibrate, nullptr); });
}
rt_status rt_multi_update_instances(rt_multi* m, const rt_instance_update* update, int recalibrate) {
    return on_every_replica(m, "rt_multi_update_instances: null rt_multi", [&](rt_scene* s) { return rt_scene_update_instances(s, update, 0, recalibrate, nullptr); });
}
rt_status rt_multi_update_quads(rt_multi* m, const rt_quad_update* update, int recalibrate) {
    return on_every_replica(m, "rt_multi_update_quads: null rt_multi", [&](rt_scene* s) { return rt_scene_update_quads(s, update, 0, recalibrate, nullptr); });
}

rt_status rt_multi_row_owner(int32_t global_row, int32_t tile_rows, int32_t n_gpus, int32_t* device, int32_t* local_row) {
    if (global_row < 0 || tile_rows <= 0 || n_gpus <= 0 || !device || !local_row) return fail(RT_ERR_INVALID, 0, "rt_multi_row_owner: bad argument");
    int r, l;
    row_owner(global_row, tile_rows, n_gpus, r, l);
    *device = r; *local_row = l;
    return RT_OK;
}

// After a failure once frames are enqueued: wait for every device and close every scene's pending frame, so that the
// replicas are usable again (and nothing still writes d_local) when the error status reaches the caller.
static void drain_devices(rt_multi* m) {
    for (int d = 0; d < m->n; ++d) {
        if (hipSetDevice(d) != hipSuccess) continue;
        if (m->streams[d]) (void)hipStreamSynchronize(m->streams[d]);
        if (m->scenes[d]) (void)rt_frame_finish(m->scenes[d], nullptr);
    }
    (void)hipSetDevice(0);
}

// buffers and communicators of a frame shape (no-ops once they are large enough / exist)
static rt_status multi_setup(rt_multi* m, size_t local_floats, size_t frame_floats, bool gather) {
    const int n = m->n;
    if (m->local_floats < local_floats) {
        for (int d = 0; d < n; ++d) {
            HIPCHK(hipSetDevice(d));
            if (m->d_local[d]) (void)hipFree(m->d_local[d]);
            m->d_local[d] = nullptr;
        }
        m->local_floats = 0;
        for (int d = 0; d < n; ++d) {
            HIPCHK(hipSetDevice(d));
            HIPCHK(hipMalloc((void**)&m->d_local[d], (local_floats ? local_floats : 1) * sizeof(float)));
        }
        m->local_floats = local_floats;
    }
    HIPCHK(hipSetDevice(0));
    if (m->frame_floats < frame_floats) {
        if (m->d_frame) (void)hipFree(m->d_frame);
        m->d_frame = nullptr; m->frame_floats = 0;
        HIPCHK(hipMalloc((void**)&m->d_frame, frame_floats * sizeof(float)));
        m->frame_floats = frame_floats;
    }
    // the gather writes n * local_floats floats of THIS frame: its capacity is tracked on its own (a frame rendered
    // without the gather allocates none)
    const size_t staging_need = gather ? (size_t)n * (local_floats ? local_floats : 1) : 0;
    if (m->staging_floats < staging_need) {
        if (m->d_staging) (void)hipFree(m->d_staging);
        m->d_staging = nullptr; m->staging_floats = 0;
        HIPCHK(hipMalloc((void**)&m->d_staging, staging_need * sizeof(float)));
        m->staging_floats = staging_need;
    }
    if (gather && !m->comms_ready) {
        std::string why;
        if (!load_rccl(m->rccl, why)) return fail(RT_ERR_HIP, 0, why);
        m->comms.assign((size_t)n, nullptr);
        std::vector<int> devs((size_t)n);
        for (int d = 0; d < n; ++d) devs[d] = d;
        const int rc = m->rccl.CommInitAll(m->comms.data(), n, devs.data());    // rccl.h:236
        if (rc != 0) return fail(RT_ERR_HIP, rc, std::string("ncclCommInitAll: ") + (m->rccl.GetErrorString ? m->rccl.GetErrorString(rc) : "failed"));
        m->comms_ready = true;
    }
    return RT_OK;
}

rt_status rt_multi_render(rt_multi* m, const rt_frame_desc* whole, float* fb, int fb_on_device, int tile_rows, rt_stats* stats) {
    if (!m || !whole || !fb) return fail(RT_ERR_INVALID, 0, "null argument");
    if (whole->nx <= 0 || whole->ny <= 0 || whole->ns <= 0) return fail(RT_ERR_INVALID, 0, "nx, ny and ns must be positive");
    const int n = m->n, nx = whole->nx, ny = whole->ny;
    const bool force_rccl = g_opt.multi_force_rccl != 0;
    const bool gather = n > 1 || force_rccl;
    if (tile_rows <= 0) tile_rows = 4;
    if (!gather) tile_rows = ny;

    // rows per device and the common (padded) buffer size of the gather
    std::vector<rt_frame_desc> f((size_t)n, *whole);
    int max_rows = 0;
    for (int d = 0; d < n; ++d) {
        f[d].tile_rows = tile_rows; f[d].tile_first = d; f[d].tile_stride = n;
        const int rows = rt_frame_local_rows(&f[d]);
        if (rows < 0) return fail(RT_ERR_INVALID, 0, "bad row partition");
        if (rows > max_rows) max_rows = rows;
    }
    const size_t local_floats = (size_t)max_rows * nx * 3, frame_floats = (size_t)ny * nx * 3;
    {   // one-time setup (allocations, dlopen, ncclCommInitAll: seconds on a first call) stays out of the frame's time
        const rt_status st = multi_setup(m, local_floats, frame_floats, gather);
        if (st != RT_OK) return st;
    }
    const auto t0 = std::chrono::steady_clock::now();
    // from here on frames are in flight: an error drains every device before it is returned
    rt_status failed = RT_OK;
    // (HIPCHK's record of the first error, without its return)
#define MTRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess && failed == RT_OK) failed = hip_failed(e_, __FILE__, __LINE__, #expr); } while (0)

    // ---- every device renders its rows (enqueue only: the devices run concurrently)
    for (int d = 0; d < n && failed == RT_OK; ++d) {
        float* dst = gather ? m->d_local[d] : m->d_frame;
        failed = rt_render(m->scenes[d], &f[d], dst, /*fb_on_device=*/1, m->streams[d], /*blocking=*/0, nullptr);
    }
    // ---- one gather to device 0 over xGMI, then the rows go to their places
    if (gather && failed == RT_OK) {
        int rc = m->rccl.GroupStart();
        for (int d = 0; d < n && rc == 0 && failed == RT_OK; ++d) {
            MTRY(hipSetDevice(d));
            if (failed == RT_OK) rc = m->rccl.Gather(m->d_local[d], d == 0 ? m->d_staging : nullptr, local_floats, NCCL_FLOAT, 0, m->comms[d], m->streams[d]);
        }
        const int rc2 = m->rccl.GroupEnd();   // always closes the group that GroupStart opened
        if (rc == 0) rc = rc2;
        if (rc != 0 && failed == RT_OK) {
            failed = fail(RT_ERR_HIP, rc, std::string("ncclGather: ") + (m->rccl.GetErrorString ? m->rccl.GetErrorString(rc) : "failed"));
        }
        if (failed == RT_OK) {
            MTRY(hipSetDevice(0));
            const long long total = (long long)ny * nx * 3;
            hipLaunchKernelGGL(rt_uninterleave_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, m->streams[0], m->d_staging, m->d_frame, nx * 3, ny, tile_rows, n, max_rows);
            MTRY(hipGetLastError());
        }
    }
    if (failed == RT_OK) {
        MTRY(hipSetDevice(0));
        MTRY(hipMemcpyAsync(fb, m->d_frame, frame_floats * sizeof(float), fb_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, m->streams[0]));
    }
    if (failed != RT_OK) { drain_devices(m); return failed; }
    // ---- wait for every device, add up the statistics
    rt_stats total_stats;
    memset(&total_stats, 0, sizeof(total_stats));
    double slowest = 0.0;
    for (int d = n - 1; d >= 0; --d) {
        MTRY(hipSetDevice(d));
        MTRY(hipStreamSynchronize(m->streams[d]));
        rt_stats st;
        memset(&st, 0, sizeof(st));
        const rt_status rs = rt_frame_finish(m->scenes[d], &st);
        if (rs != RT_OK && failed == RT_OK) failed = rs;
        total_stats.rays += st.rays; total_stats.samples += st.samples; total_stats.local_rows += st.local_rows;
        total_stats.workgroups += st.workgroups;
        if (st.ms_render > slowest) slowest = st.ms_render;
        if (d == 0) { total_stats.kernel_variant = st.kernel_variant; total_stats.threads_per_group = st.threads_per_group; total_stats.lds_bytes = st.lds_bytes; }
    }
#undef MTRY
    if (failed != RT_OK) { drain_devices(m); return failed; }
    const double wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // ms_render: host wall time of the whole multi-device frame (render on every device + gather + reassembly + the copy
    // into fb; one-time setup excluded); the slowest device's own render time is in `reserved` (microseconds)
    total_stats.ms_render = wall_ms;
    total_stats.reserved = (int32_t)(slowest * 1000.0);
    if (stats) *stats = total_stats;
    return RT_OK;
}

// ---- test hooks (declared in include/rt_abi.h under "diagnostics")
// Tries to load RCCL the way rt_multi_render does -- from `library_name` only when one is given.  No device involved:
// a missing library is an error status with the loader's message, never a crash.
rt_status rt_multi_probe_rccl(const char* library_name) {
    rccl_api r;
    std::string why;
    if (!load_rccl(r, why, library_name)) return fail(RT_ERR_HIP, 0, why);
    dlclose(r.handle);
    return RT_OK;
}
// The reassembly step of rt_multi_render on caller-supplied DEVICE buffers: staging[world][max_rows][nx*3] -> frame[ny][nx*3]
// on the current device's default stream (synchronous).  Lets a one-GPU box check the index arithmetic for any world size.
rt_status rt_multi_debug_uninterleave(const float* staging, float* frame, int32_t nx, int32_t ny, int32_t tile_rows, int32_t world, int32_t max_rows) {
    if (!staging || !frame || nx <= 0 || ny <= 0 || tile_rows <= 0 || world <= 0 || max_rows <= 0) return fail(RT_ERR_INVALID, 0, "rt_multi_debug_uninterleave: bad argument");
    const long long total = (long long)ny * nx * 3;
    hipLaunchKernelGGL(rt_uninterleave_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, staging, frame, nx * 3, ny, tile_rows, world, max_rows);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return RT_OK;
}

}  // extern "C"
