// vrt_edit.hip — batched voxel inserts behind the C ABI (vrt_insert_voxels, vrt_insert_voxels_device), the allocation state they
// continue (vrt_scene_bricks) and the read-back of a scene buffer (vrt_read_buffer).  BrickGrid.insert (Grid.zig:129-194) for a whole
// batch, on the context's scene buffers, with the bytes a vrt_grid gives after vrt_grid_insert_many; a failed batch writes nothing.
// The kernels live in a code object of their own next to the library (vrt_edit_kernel.hip -> vrt_edit.hsaco), loaded on a context's
// first insert with hipModuleLoad and unloaded by vrt_destroy.  The library keeps no other dependency on it: without the file, frames
// and queries work and inserts fail with VRT_E_STATE.  DESIGN.md §11.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <unistd.h>
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include "vrt_ctx.h"
#include "vrt_edit.h"

using namespace vrt_impl;

namespace {

enum EditKernel { K_BEGIN, K_SCAN_START, K_STATE, K_VALIDATE, K_COUNT, K_SCAN_GROUPS, K_RANK, K_RESOLVE, K_TABLE, K_WRITE, K_FINISH, K_KERNELS };
const char *const kEditKernelNames[K_KERNELS] = {"vrt_edit_begin",  "vrt_edit_scan_start", "vrt_edit_state",   "vrt_edit_validate",
                                                "vrt_edit_count",  "vrt_edit_scan_groups", "vrt_edit_rank",   "vrt_edit_resolve",
                                                "vrt_edit_table",  "vrt_edit_write",      "vrt_edit_finish"};
static_assert(K_KERNELS == sizeof(((vrt_ctx *)nullptr)->edit_fn) / sizeof(hipFunction_t), "one function slot per edit kernel");

// the edit code object: vrt_edit.hsaco in the library's own directory
std::string code_object_path() {
    Dl_info info{};
    std::string dir = ".";
    if (dladdr(reinterpret_cast<void *>(&vrt_impl::edit_release), &info) && info.dli_fname) {
        const std::string lib = info.dli_fname;
        const size_t slash = lib.rfind('/');
        if (slash != std::string::npos) dir = lib.substr(0, slash);
    }
    return dir + "/vrt_edit.hsaco";
}

int load_edit_kernels(vrt_ctx *ctx) {
    if (ctx->edit_module) return VRT_OK;
    const std::string path = code_object_path();
    if (access(path.c_str(), R_OK) != 0) return fail(ctx, VRT_E_STATE, "voxel-edit code object missing: " + path);
    hipModule_t m = nullptr;
    const hipError_t e = hipModuleLoad(&m, path.c_str());
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, VRT_E_STATE, "voxel-edit code object " + path + " did not load: " + hipGetErrorString(e));
    }
    for (int k = 0; k < K_KERNELS; k++) {
        const hipError_t ef = hipModuleGetFunction(&ctx->edit_fn[k], m, kEditKernelNames[k]);
        if (ef != hipSuccess) {
            (void)hipGetLastError();
            (void)hipModuleUnload(m);
            std::fill(ctx->edit_fn, ctx->edit_fn + K_KERNELS, nullptr);
            return fail(ctx, VRT_E_STATE, "voxel-edit code object " + path + " lacks " + kEditKernelNames[k] + ": " + hipGetErrorString(ef));
        }
    }
    ctx->edit_module = m;
    return VRT_OK;
}

// what every entry point checks before it touches the device: the scene is there, this context may edit it, the kernels are loaded,
// and the small buffers of the allocation state exist
int edit_prepare(vrt_ctx *ctx) {
    if (ctx->dist) return fail(ctx, VRT_E_STATE, "voxel inserts are not available on a context of the multi-GPU pipeline");
    if (!ctx->grid_uploaded) return fail(ctx, VRT_E_STATE, "no grid state uploaded yet (vrt_upload_grid)");
    const int rc = load_edit_kernels(ctx);
    if (rc != VRT_OK) return rc;
    if (!ctx->d_edit_state) {
        VRT_HIP(ctx, ctx->res.device(&ctx->d_edit_state, sizeof(vrt::EditState)));
        VRT_HIP(ctx, ctx->res.device(&ctx->d_edit_status, sizeof(vrt::EditStatus)));
        VRT_HIP(ctx, ctx->res.pinned(&ctx->h_edit_status, sizeof(vrt::EditStatus)));
    }
    return VRT_OK;
}

// scratch for a batch of n voxels: the per-cell words (once, all 0xFFFFFFFF; every batch leaves them so), the per-voxel words, the
// per-workgroup counts and the last-writer table (a power of two of at least 2n entries).  No kernel of an earlier batch is in flight:
// every batch ends with a wait for its status.
int edit_scratch(vrt_ctx *ctx, uint64_t n) {
    if (!ctx->d_edit_cell_first) {
        const uint64_t cells = (uint64_t)ctx->cfg.dim_x * ctx->cfg.dim_y * ctx->cfg.dim_z;
        VRT_HIP(ctx, ctx->res.device(&ctx->d_edit_cell_first, cells * sizeof(uint32_t)));
        VRT_HIP(ctx, hipMemsetAsync(ctx->d_edit_cell_first, 0xFF, cells * sizeof(uint32_t), ctx->stream));
    }
    if (ctx->edit_capacity < n) {
        const uint64_t cap = (n + vrt::kEditBlock - 1u) / vrt::kEditBlock * vrt::kEditBlock;
        ctx->res.drop(ctx->d_edit_voxels);
        ctx->res.drop(ctx->d_edit_groups);
        ctx->edit_capacity = 0;
        VRT_HIP(ctx, ctx->res.device(&ctx->d_edit_voxels, 4u * cap * sizeof(uint32_t)));
        VRT_HIP(ctx, ctx->res.device(&ctx->d_edit_groups, cap / vrt::kEditBlock * sizeof(uint32_t)));
        ctx->edit_capacity = cap;
    }
    uint64_t entries = 1024;
    while (entries < 2u * n) entries <<= 1;
    if (ctx->edit_table_entries < entries) {
        ctx->res.drop(ctx->d_edit_table);
        ctx->edit_table_entries = 0;
        VRT_HIP(ctx, ctx->res.device(&ctx->d_edit_table, entries * sizeof(uint2)));
        ctx->edit_table_entries = entries;
    }
    return VRT_OK;
}

vrt::EditArgs edit_args(vrt_ctx *ctx, const uint32_t *xyz, const uint8_t *materials, uint32_t n, bool rescan) {
    vrt::EditArgs a{};
    a.status = static_cast<uint32_t *>(ctx->dbuf[VRT_BUF_BRICK_STATUS]);
    a.index = static_cast<uint32_t *>(ctx->dbuf[VRT_BUF_BRICK_INDEX]);
    a.occupancy = static_cast<uint32_t *>(ctx->dbuf[VRT_BUF_BRICK_OCCUPANCY]);
    a.start = static_cast<uint32_t *>(ctx->dbuf[VRT_BUF_BRICK_START_INDEX]);
    a.material = static_cast<uint8_t *>(ctx->dbuf[VRT_BUF_MATERIAL_INDEX]);
    a.xyz = xyz;
    a.materials = materials;
    a.n = n;
    a.groups = (n + vrt::kEditBlock - 1u) / vrt::kEditBlock;
    a.rescan = rescan ? 1u : 0u;
    a.cell_first = ctx->d_edit_cell_first;
    const uint64_t cap = ctx->edit_capacity;
    a.vcell = ctx->d_edit_voxels;
    a.vinfo = ctx->d_edit_voxels ? ctx->d_edit_voxels + cap : nullptr;
    a.vbrick = ctx->d_edit_voxels ? ctx->d_edit_voxels + 2u * cap : nullptr;
    a.vslot = ctx->d_edit_voxels ? ctx->d_edit_voxels + 3u * cap : nullptr;
    a.group_sums = ctx->d_edit_groups;
    a.table = static_cast<uint2 *>(ctx->d_edit_table);
    a.table_mask = ctx->edit_table_entries ? (uint32_t)(ctx->edit_table_entries - 1u) : 0u;
    a.state = ctx->d_edit_state;
    a.out = ctx->d_edit_status;
    const uint32_t b = ctx->cfg.brick_dimension;
    a.voxel_dim_x = ctx->cfg.dim_x * b;
    a.voxel_dim_y = ctx->cfg.dim_y * b;
    a.voxel_dim_z = ctx->cfg.dim_z * b;
    a.dim_x = ctx->cfg.dim_x;
    a.dim_z = ctx->cfg.dim_z;
    a.b = b;
    a.bits = b * b * b;
    a.brick_bytes = a.bits / 8u;
    a.brick_alloc = (uint32_t)(ctx->dsize[VRT_BUF_BRICK_START_INDEX] / 4u);
    a.start_words = a.brick_alloc;
    a.material_entries = ctx->dsize[VRT_BUF_MATERIAL_INDEX];
    return a;
}

int launch(vrt_ctx *ctx, EditKernel k, vrt::EditArgs &a, uint32_t groups, uint32_t threads) {
    if (groups == 0) return VRT_OK;
    size_t bytes = sizeof a;
    void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
    (void)hipGetLastError(); // (the thread's stale error is not this launch's)
    VRT_HIP(ctx, hipModuleLaunchKernel(ctx->edit_fn[k], groups, 1, 1, threads, 1, 1, 0, ctx->stream, nullptr, config));
    return VRT_OK;
}

// the head of every chain: the batch's status cleared and, after a write to binding 5, the allocation state computed from it
int launch_state(vrt_ctx *ctx, vrt::EditArgs &a) {
    int rc = launch(ctx, K_BEGIN, a, 1, 64);
    if (rc == VRT_OK && a.rescan) {
        const uint32_t groups = std::max<uint32_t>(1u, std::min<uint32_t>((a.start_words + vrt::kEditBlock - 1u) / vrt::kEditBlock, 2048u));
        rc = launch(ctx, K_SCAN_START, a, groups, vrt::kEditBlock);
        if (rc == VRT_OK) rc = launch(ctx, K_STATE, a, 1, 64);
    }
    return rc;
}

// the tail of every chain: the status back to the host (the one read-back), and the host's copy of the state
int read_status(vrt_ctx *ctx, vrt::EditArgs &a, vrt::EditStatus *out) {
    int rc = launch(ctx, K_FINISH, a, 1, 64);
    if (rc != VRT_OK) return rc;
    VRT_HIP(ctx, hipMemcpyAsync(ctx->h_edit_status, ctx->d_edit_status, sizeof(vrt::EditStatus), hipMemcpyDeviceToHost, ctx->stream));
    VRT_HIP(ctx, wait_stream(ctx->stream));
    *out = *ctx->h_edit_status;
    ctx->edit_state_valid = true;
    ctx->edit_ok = out->ok != 0;
    ctx->edit_bricks = out->bricks;
    ctx->edit_cursor = out->cursor;
    return VRT_OK;
}

int not_shaped(vrt_ctx *ctx) {
    return fail(ctx, VRT_E_STATE, "binding 5 (brick_start_indices) is not allocation-shaped: entries [0, A) set with type bit 0, the rest "
                                  "0xFFFFFFFF, and the largest start + B^3 within binding 6 (vrt_upload_grid makes it so)");
}

// n voxels at xyz / materials (device memory) into the scene: the whole chain on the primary stream as one scene write
int insert(vrt_ctx *ctx, const uint32_t *xyz, const uint8_t *materials, uint64_t n) {
    if (ctx->edit_state_valid && !ctx->edit_ok) return not_shaped(ctx); // (nothing to launch: the state has not changed)
    int rc = edit_scratch(ctx, n);
    if (rc != VRT_OK) return rc;
    rc = begin_scene_write(ctx);
    if (rc != VRT_OK) return rc;
    vrt::EditArgs a = edit_args(ctx, xyz, materials, (uint32_t)n, !ctx->edit_state_valid);
    const uint32_t groups = a.groups;
    VRT_HIP(ctx, hipMemsetAsync(ctx->d_edit_table, 0, ctx->edit_table_entries * sizeof(uint2), ctx->stream));
    rc = launch_state(ctx, a);
    if (rc == VRT_OK) rc = launch(ctx, K_VALIDATE, a, groups, vrt::kEditBlock);
    if (rc == VRT_OK) rc = launch(ctx, K_COUNT, a, groups, vrt::kEditBlock);
    if (rc == VRT_OK) rc = launch(ctx, K_SCAN_GROUPS, a, 1, vrt::kEditScanBlock);
    if (rc == VRT_OK) rc = launch(ctx, K_RANK, a, groups, vrt::kEditBlock);
    if (rc == VRT_OK) rc = launch(ctx, K_RESOLVE, a, groups, vrt::kEditBlock);
    if (rc == VRT_OK) rc = launch(ctx, K_TABLE, a, groups, vrt::kEditBlock);
    if (rc == VRT_OK) rc = launch(ctx, K_WRITE, a, groups, vrt::kEditBlock);
    if (rc != VRT_OK) {
        (void)wait_stream(ctx->stream);
        ctx->res.drop(ctx->d_edit_cell_first); // (a chain cut short may leave scratch words set: made anew, clean, by the next batch)
        ctx->edit_state_valid = false;
        return rc;
    }
    rc = end_scene_write(ctx);
    if (rc != VRT_OK) return rc;
    vrt::EditStatus s;
    rc = read_status(ctx, a, &s);
    if (rc != VRT_OK) return rc;
    if (s.err & vrt::kEditErrShape) return not_shaped(ctx);
    if (s.err & vrt::kEditErrRange) return fail(ctx, VRT_E_OUT_OF_RANGE, "a voxel lies outside the grid; nothing was inserted");
    if (s.err & vrt::kEditErrCell)
        return fail(ctx, VRT_E_STATE, "a loaded cell names a brick at or beyond the allocated bricks (binding 3 against binding 5); nothing was inserted");
    if (s.err & vrt::kEditErrOom)
        return fail(ctx, VRT_E_OOM, "the batch needs " + std::to_string(s.new_bricks) + " new bricks: brick_alloc or the material entries are exhausted; nothing was inserted");
    // the derived structures follow exactly what was written (refresh_derived, before the next frame or query)
    const uint64_t bpw = 4u;
    if (s.cell_lo <= s.cell_hi) {
        mark_dirty(ctx, VRT_BUF_BRICK_STATUS, (uint64_t)(s.cell_lo >> 5) * bpw, (uint64_t)((s.cell_hi >> 5) - (s.cell_lo >> 5) + 1u) * bpw);
        mark_dirty(ctx, VRT_BUF_BRICK_INDEX, (uint64_t)s.cell_lo * bpw, ((uint64_t)s.cell_hi - s.cell_lo + 1u) * bpw);
    }
    if (s.occ_lo <= s.occ_hi) mark_dirty(ctx, VRT_BUF_BRICK_OCCUPANCY, s.occ_lo, (uint64_t)s.occ_hi - s.occ_lo + 1u);
    if (s.new_bricks) {
        mark_dirty(ctx, VRT_BUF_BRICK_START_INDEX, (uint64_t)(s.bricks - s.new_bricks) * bpw, (uint64_t)s.new_bricks * bpw);
        ctx->edit_state_valid = true; // (the device state already counts these bricks: this write is the inserts' own)
    }
    if (s.mat_lo <= s.mat_hi) mark_dirty(ctx, VRT_BUF_MATERIAL_INDEX, s.mat_lo, (uint64_t)s.mat_hi - s.mat_lo + 1u);
    return VRT_OK;
}

int check_batch(vrt_ctx *ctx, const uint32_t *xyz, const uint8_t *materials, uint64_t n) {
    if (!xyz || !materials) return fail(ctx, VRT_E_INVALID_ARG, "xyz or materials is NULL");
    if (n >= (1ull << 31)) return fail(ctx, VRT_E_OUT_OF_RANGE, "a batch holds fewer than 2^31 voxels");
    return VRT_OK;
}

} // namespace

namespace vrt_impl {
void edit_release(vrt_ctx *ctx) {
    if (!ctx->edit_module) return;
    (void)hipModuleUnload(ctx->edit_module);
    ctx->edit_module = nullptr;
    std::fill(ctx->edit_fn, ctx->edit_fn + K_KERNELS, nullptr);
}
} // namespace vrt_impl

extern "C" {

int vrt_insert_voxels_device(vrt_ctx *ctx, const uint32_t *xyz, const uint8_t *materials, uint64_t n) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if (n == 0) return VRT_OK;
    int rc = check_batch(ctx, xyz, materials, n);
    if (rc != VRT_OK) return rc;
    DeviceGuard dg(ctx->device);
    rc = edit_prepare(ctx);
    if (rc != VRT_OK) return rc;
    return insert(ctx, xyz, materials, n);
}

int vrt_insert_voxels(vrt_ctx *ctx, const uint32_t *xyz, const uint8_t *materials, uint64_t n) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if (n == 0) return VRT_OK;
    int rc = check_batch(ctx, xyz, materials, n);
    if (rc != VRT_OK) return rc;
    DeviceGuard dg(ctx->device);
    rc = edit_prepare(ctx);
    if (rc != VRT_OK) return rc;
    // the batch into device memory through the pinned staging slots (xyz, then the material bytes behind it)
    const uint64_t xyz_bytes = 12u * n, bytes = xyz_bytes + n;
    if (ctx->edit_input_bytes < bytes) {
        ctx->res.drop(ctx->d_edit_input);
        ctx->edit_input_bytes = 0;
        VRT_HIP(ctx, ctx->res.device(&ctx->d_edit_input, bytes));
        ctx->edit_input_bytes = bytes;
    }
    rc = staged_copy_h2d(ctx, ctx->d_edit_input, xyz, xyz_bytes);
    if (rc == VRT_OK) rc = staged_copy_h2d(ctx, ctx->d_edit_input + xyz_bytes, materials, n);
    if (rc != VRT_OK) return rc;
    return insert(ctx, reinterpret_cast<const uint32_t *>(ctx->d_edit_input), ctx->d_edit_input + xyz_bytes, n);
}

int vrt_scene_bricks(vrt_ctx *ctx, uint32_t out[2]) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if (!out) return fail(ctx, VRT_E_INVALID_ARG, "out is NULL");
    DeviceGuard dg(ctx->device);
    int rc = edit_prepare(ctx);
    if (rc != VRT_OK) return rc;
    if (!ctx->edit_state_valid) {
        vrt::EditArgs a = edit_args(ctx, nullptr, nullptr, 0, true);
        rc = launch_state(ctx, a);
        if (rc != VRT_OK) return rc;
        vrt::EditStatus s;
        rc = read_status(ctx, a, &s);
        if (rc != VRT_OK) return rc;
    }
    if (!ctx->edit_ok) return not_shaped(ctx);
    out[0] = ctx->edit_bricks;
    out[1] = (uint32_t)ctx->edit_cursor;
    return VRT_OK;
}

int vrt_read_buffer(vrt_ctx *ctx, vrt_buffer_id id, uint64_t byte_offset, void *dst, uint64_t nbytes) {
    if (!ctx) return VRT_E_INVALID_ARG;
    if ((int)id < 0 || id >= VRT_BUF_COUNT) return fail(ctx, VRT_E_INVALID_ARG, "bad buffer id");
    if (nbytes && !dst) return fail(ctx, VRT_E_INVALID_ARG, "dst is NULL");
    if (byte_offset > ctx->dsize[id] || nbytes > ctx->dsize[id] - byte_offset) return fail(ctx, VRT_E_OUT_OF_RANGE, "read exceeds the device buffer");
    if (nbytes == 0) return VRT_OK;
    DeviceGuard dg(ctx->device);
    // (the primary stream holds every scene write; frames read the scene, they do not write it)
    VRT_HIP(ctx, hipMemcpyAsync(dst, static_cast<const uint8_t *>(ctx->dbuf[id]) + byte_offset, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    VRT_HIP(ctx, wait_stream(ctx->stream));
    return VRT_OK;
}

} // extern "C"
