// stmmqr_host.cpp -- what libstmmqr_hip.so holds process-wide: the globals, the error message, the options, device set-up with the
// side stream of the look-ahead schedule, device alloc / copy / free and shutdown.  The plan is built in stmmqr_planbuild.cpp,
// scheduled in stmmqr_schedule.cpp, factorized by stmmqr_factorize.cpp (which runs the schedule through stmmqr_run.cpp) and read
// back by stmmqr_download.cpp; the environment knobs are the table of stmmqr_knobs.h.
//
// Reference counterpart (path relative to /root/reference/STMMQR):
//   qr_factorize            the drop-in seam                                include/SparseQR.h:127-135
//
// There is NO CPU fallback in this file: every numeric operation is a kernel of the stmmqr_*.hip translation units.  If no
// gfx950 device is usable the entry points fail with STMMQR_ERR_DEVICE.
#include "stmmqr_plan.h"

#include <functional>
#include <string>

thread_local std::string g_err;
stmmqr_options g_opt = {STM_NB, 64, 0, 0, 0, 1, STM_TALL_MIN, 2, 0, 4};      // (panel_algo 0: by panel height; lookahead 2: passenger launches)
size_t g_chunk[4] = {32, 5000, 4, 4};     // FCHUNK, SMALL, MINCHUNK, MINCHUNK_RATIO (SparseQR.h:16-19)

stm_common_layout g_layout = {
    /* status */ 1004, /* malloc_count */ 1032, /* memory_usage */ 1040, /* memory_inuse */ 1048,
    /* blas_ok */ 1100, /* SPQR_grain */ 1104, /* SPQR_small */ 1112, /* SPQR_shrink */ 1120,
    /* SPQR_flopcount */ 1128, /* SPQR_flopcount_bound */ 1136};

int fail(int code, const std::string &msg)
{
    g_err = msg;
    if (g_opt.verbose) fprintf(stderr, "[stmmqr_hip] error %d: %s\n", code, msg.c_str());
    return code;
}

int stm_ensure_device(int device)
{
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0)
        return fail(STMMQR_ERR_DEVICE, "no HIP device visible: the MI355X path has no CPU fallback");
    if (device >= cnt) return fail(STMMQR_ERR_DEVICE, "device index out of range");
    if (device >= 0) HIPCHK(hipSetDevice(device));
    static bool configured = false;
    if (!configured) {
        LCHK(stm_configure_kernels());
        LCHK(stm_configure_capanel());
        configured = true;
    }
    return 0;
}

// The side stream of the look-ahead schedule: ONE per device and process, created at the first look-ahead factorization
// and kept (a CU-masked stream owns a hardware queue; creating one per plan exhausted them).  Its CU mask leaves
// STMMQR_SIDE_RESERVE compute units (the mask bits interleave over the 8 XCDs, so 4 per XCD at 32) to the plan
// streams: the workgroups of a panel kernel need most of a CU's LDS and would otherwise wait until the side stream's
// update grid has drained.  Plans of one device that factorize at the same time share it (still ordered by events).
static std::mutex g_side_mu;
static hipStream_t g_side[64] = {};
static bool g_side_tried[64] = {};

// (registered with atexit at the first creation, i.e. after the HIP runtime registered its own handlers: it runs before
//  them; stmmqr_shutdown() calls it too)
void stm_destroy_side_streams()
{
    std::lock_guard<std::mutex> lock(g_side_mu);
    for (int d = 0; d < 64; d++) {
        if (g_side[d]) {
            if (hipSetDevice(d) == hipSuccess) { (void)hipStreamSynchronize(g_side[d]); (void)hipStreamDestroy(g_side[d]); }
            g_side[d] = nullptr;
        }
        g_side_tried[d] = false;
    }
}

hipStream_t stm_side_stream_for(int device)
{
    hipStream_t *side = g_side;
    bool *tried = g_side_tried;
    static bool registered = false;
    if (device < 0 || device >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(g_side_mu);
    if (tried[device]) return side[device];
    tried[device] = true;
    if (!registered) { registered = true; atexit(stm_destroy_side_streams); }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return nullptr;
    const int ncu = prop.multiProcessorCount;
    int reserve = (int)knobs::num(knobs::K_SIDE_RESERVE);
    if (reserve > ncu / 2) reserve = ncu / 2;
    hipStream_t q = nullptr;
    if (reserve > 0) {
        std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
        for (int i = reserve; i < ncu; i++) mask[(size_t)i >> 5] |= 1u << (i & 31);
        if (hipExtStreamCreateWithCUMask(&q, (uint32_t)mask.size(), mask.data()) != hipSuccess) q = nullptr;
    }
    if (!q && hipStreamCreateWithFlags(&q, hipStreamNonBlocking) != hipSuccess) q = nullptr;
    side[device] = q;
    return q;
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

const char *stmmqr_version(void) { return "stmmqr_hip 0.1 (gfx950)"; }
const char *stmmqr_last_error(void) { return g_err.c_str(); }
void stmmqr_get_options(stmmqr_options *o) { if (o) *o = g_opt; }
void stmmqr_set_options(const stmmqr_options *o)
{
    if (!o) return;
    g_opt = *o;
    if (g_opt.big_front_cols < 1) g_opt.big_front_cols = 1;
}
void stmmqr_set_common_layout(const stm_common_layout *l) { if (l) g_layout = *l; }
void stmmqr_get_common_layout(stm_common_layout *l) { if (l) *l = g_layout; }

/* End of use (optional): waits for the device and releases what the library holds process-wide.  A host program that
 * dlopen()s the library calls it before returning from main; the library has no static object whose destructor calls
 * into the HIP runtime, so nothing else happens at exit / dlclose. */
int stmmqr_device_alloc(size_t bytes, void **ptr)
{
    if (!ptr) return fail(STMMQR_ERR_INVALID, "null argument");
    *ptr = nullptr;
    if (hipMalloc(ptr, bytes ? bytes : 1) != hipSuccess) return fail(STMMQR_ERR_OUT_OF_MEMORY, "hipMalloc failed");
    return 0;
}
/* device-to-device copy, complete on return (after everything `hip_stream` -- may be NULL -- held before it); for callers that
 * implement a stmmqr_transport of their own on one GPU (tests).  With a stream the copy is a command OF that stream: what the
 * library records on the stream after the transport's call (the event its compute stream waits for before it unpacks a panel
 * message) then orders the copy's writes before the kernels that read them.  As a null-stream copy beside an empty stream that
 * event carried no dependency on the copy, and the unpacking kernel now and then read the PREVIOUS message of a reused ring
 * buffer (thread ranks on one GPU: a shared front wrong from one panel on, one run in two of the sharded tests). */
int stmmqr_device_copy(void *dst, const void *src, size_t bytes, void *hip_stream)
{
    if (hip_stream) {
        if (bytes) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)hip_stream));
    } else if (bytes) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
    HIPCHK(hipDeviceSynchronize());
    return 0;
}
int stmmqr_device_free(void *ptr)
{
    if (ptr && hipFree(ptr) != hipSuccess) return fail(STMMQR_ERR_DEVICE, "hipFree failed");
    return 0;
}

void stmmqr_plan_cache_clear(void);
void stmmqr_shutdown(void)
{
    stmmqr_plan_cache_clear();
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) == hipSuccess && cnt > 0) {
        (void)hipDeviceSynchronize();
        int dev = 0;
        (void)hipGetDevice(&dev);
        stm_destroy_side_streams();
        (void)hipSetDevice(dev);
    }
}

int stmmqr_device_count(void)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}
const char *stmmqr_device_name(int device)
{
    static thread_local char name[256];
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return "";
    snprintf(name, sizeof name, "%s", prop.gcnArchName);
    return name;
}

int chunk_getSettings(size_t a, size_t b, size_t c, size_t d)
{
    g_chunk[0] = a; g_chunk[1] = b; g_chunk[2] = c; g_chunk[3] = d;
    return 0;
}

}  // extern "C"
