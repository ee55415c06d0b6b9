// error reporting, version and host-side launch helpers for libxggm_hip.so
#include "common.h"
#include "xggm.h"
#include <map>
#include <mutex>

static thread_local char g_err[512] = "";

void xggm_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int xggm_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        xggm_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
        return XGGM_ERR_LAUNCH;
    }
    return XGGM_OK;
}

extern "C" int xggm_version(void) { return XGGM_VERSION; }
extern "C" const char* xggm_last_error(void) { return g_err; }

int xggm_prefetch_args(const xggm_prefetch* r, PrefetchArgs* a, const char* who) {
    *a = PrefetchArgs{};
    if (!r) return XGGM_OK;
    XGGM_REQUIRE(r->n >= 0 && r->n <= 4, "%s: %d prefetch ranges (0..4)", who, r->n);
    unsigned long long total = 0;
    for (int i = 0; i < r->n; ++i) {
        XGGM_REQUIRE(r->ptr[i] && reinterpret_cast<uintptr_t>(r->ptr[i]) % 16 == 0 && r->bytes[i] >= 16,
                     "%s: prefetch range %d must be non-null, start on a 16-byte border and hold at least 16 bytes", who, i);
        a->p[i] = r->ptr[i]; a->n[i] = r->bytes[i];
        total += a->n[i];
    }
    a->k = r->n;
    a->blocks = (int)std::min<unsigned long long>(256, (total + 49151) / 49152);  // ~48 KB per workgroup, at most one per CU
    return XGGM_OK;
}

int xggm_reserve_lds(const void* kernel, size_t bytes, const char* who) {
    if (bytes <= 48 * 1024) return XGGM_OK;
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, size_t> granted;  // (kernel, device) -> largest reservation so far
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lock(mu);
        size_t& have = granted[{kernel, dev}];
        if (bytes > have) {
            e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
            if (e == hipSuccess) have = bytes;
        }
    }
    if (e != hipSuccess) {
        xggm_set_error("%s: cannot reserve %zu bytes of LDS: %s", who, bytes, hipGetErrorString(e));
        return XGGM_ERR_LAUNCH;
    }
    return XGGM_OK;
}
