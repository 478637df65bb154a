// Error string, version, device check and the diagnostic knobs behind the C ABI (include/graphpope_hip.h).
#include <cstring>

#include "common.h"

namespace pope {

static thread_local char g_error[512] = "";

void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

void clear_error() { g_error[0] = '\0'; }

int g_fail_host_register = 0;            // POPE_KNOB_FAIL_HOST_REGISTER, read by host.cc -- which also links without this library (tools/host_race_harness) and so cannot own it

}  // namespace pope

extern "C" const char *pope_last_error(void) { return pope::g_error; }

extern "C" const char *pope_version(void) { return "graphpope_hip 0.2 gfx950"; }

extern "C" int pope_require_device(int32_t *cu_count_host) {
    pope::clear_error();
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        pope::set_error("no gfx950 device visible (%s)", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
        return POPE_ERR_NO_DEVICE;
    }
    int dev = 0;
    POPE_HIP(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    POPE_HIP(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        pope::set_error("device %d is %s, this library is built for gfx950 only", dev, prop.gcnArchName);
        return POPE_ERR_NO_DEVICE;
    }
    if (cu_count_host) *cu_count_host = prop.multiProcessorCount;
    return POPE_OK;
}

// The diagnostic knobs of every module (common.h declares them; include/graphpope_hip.h documents the numbers and values).
extern "C" int pope_debug_set(int32_t knob, int32_t value) {
    pope::clear_error();
    pope::FinalizeKnobs &fin = pope::g_geodesic.fin;
    switch (knob) {
    case POPE_KNOB_LIVE_MODE:        pope::g_geodesic.live_mode = value; break;
    case POPE_KNOB_FINALIZE_VARIANT:                                 // 8 / 9 / 10: the default kernels, wide rows on the table kernel without features only / always / never
        if (value >= 8 && value <= 10) { fin.variant = 1; fin.lut = value == 9 ? 2 : value == 8 ? 1 : 0; }
        else if (value == 11 || value == 12) fin.shard_batches = value == 11;     // k_finalize_lut's batch order over several shards
        else fin.variant = value;
        break;
    case POPE_KNOB_FINALIZE_BLOCKS:  fin.blocks = value > 0 ? value : 256 * 8; fin.blocks_set = value > 0; break;
    case POPE_KNOB_PAIRWISE_KERNEL:  pope::g_pairwise_kernel = value; break;
    case POPE_KNOB_COPY_BATCHES:     pope::g_copy_batches_per_wave = value; break;
    case POPE_KNOB_FAIL_HOST_REGISTER: pope::g_fail_host_register = value; break;
    case POPE_KNOB_SAGE_FORWARD_OVERLAP: pope::g_sage_forward_overlap = value != 0; break;
    case POPE_KNOB_GEMM_TILE16_BUFFERS: pope::g_gemm_tile16_buffers = value == 4 ? 4 : 3; break;
    case POPE_KNOB_FORWARD_WHOLE_TILES: pope::g_forward_whole_tiles = value != 0; break;
    case POPE_KNOB_PREPARE_MERGE:    pope::g_geodesic.prepare_merge = value; break;
    case POPE_KNOB_LEVEL1_APPLY:     pope::g_geodesic.level1_apply = value != 0; break;
    case POPE_KNOB_LEVEL_COMPACT:    pope::g_geodesic.level_compact = value < 0 ? 0 : value > 64 ? 64 : value; break;
    case POPE_KNOB_STREAMK_XCD:      pope::g_streamk_xcd = value != 0; break;
    default: pope::set_error("pope_debug_set: unknown knob %d", knob); return POPE_ERR_INVALID;
    }
    return POPE_OK;
}

extern "C" int pope_copy_2d_to_host(const void *src, int64_t src_pitch_bytes, void *dst_host, int64_t dst_pitch_bytes,
                                    int64_t row_bytes, int64_t rows, void *stream) {
    pope::clear_error();
    POPE_REQUIRE(src && dst_host, "pope_copy_2d_to_host: null pointer");
    POPE_REQUIRE(row_bytes > 0 && rows > 0 && src_pitch_bytes >= row_bytes && dst_pitch_bytes >= row_bytes, "pope_copy_2d_to_host: bad size");
    POPE_HIP(hipMemcpy2DAsync(dst_host, (size_t)dst_pitch_bytes, src, (size_t)src_pitch_bytes, (size_t)row_bytes, (size_t)rows,
                              hipMemcpyDeviceToHost, (hipStream_t)stream));
    return POPE_OK;
}
