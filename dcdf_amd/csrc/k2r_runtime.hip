// k2r_runtime.hip -- C ABI, the calls that belong to no session (include/dcdf_k2r.h).  Host code only.
#include <mutex>
#include <string>

#include "k2r_runtime.h"

namespace k2r {

Runtime& Runtime::get() {
    static Runtime rt;
    static std::once_flag once;
    std::call_once(once, [] {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return;
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) != hipSuccess) return;
        rt.device = dev;
        rt.cus = p.multiProcessorCount;
        rt.name = std::string(p.gcnArchName) + " " + p.name + ", " + std::to_string(p.multiProcessorCount) + " CUs";
        rt.ok = true;
    });
    return rt;
}

}  // namespace k2r

extern "C" const char* dcdf_strerror(int code) {
    switch (code) {
        case DCDF_OK: return "ok";
        case DCDF_ERR_BAD_ARG: return "bad argument";
        case DCDF_ERR_NONFINITE: return "cannot convert a non-finite float to fixed point (fixed.rs:39-41)";
        case DCDF_ERR_PRECISION: return "fixed-point conversion loses precision and round is false (fixed.rs:47-59)";
        case DCDF_ERR_OVERFLOW: return "fixed-point value overflows i64 (fixed.rs:65-70)";
        case DCDF_ERR_BOUNDS: return "query out of bounds";
        case DCDF_ERR_TOO_MANY_LOGS: return "too many logs in one block (block.rs:27-32)";
        case DCDF_ERR_FORMAT: return "malformed encoded chunk";
        case DCDF_ERR_UNSUPPORTED: return "unsupported: sidelen above 1024 (universal kernel's limit; the fused kernel covers k = 2, sidelen 16..256)";
        case DCDF_ERR_NO_DEVICE: return "no usable gfx950 device / HIP failure";
        case DCDF_ERR_NOMEM: return "out of memory";
        case DCDF_ERR_CAPACITY: return "result buffer too small";
        case DCDF_ERR_INTERNAL: return "internal consistency guard tripped in a kernel (bug; see stderr)";
        case DCDF_ERR_HIP: return "HIP runtime failure (see dcdf_last_hip_error)";
        case DCDF_ERR_HIP_INVALID: return "HIP rejected an argument (bad device pointer or value)";
    }
    return "unknown error";
}
extern "C" const char* dcdf_device_name(void) {
    k2r::Runtime& rt = k2r::Runtime::get();
    return rt.ok ? rt.name.c_str() : nullptr;
}
extern "C" int dcdf_abi_version(void) { return 3; }
extern "C" int dcdf_device_pool_trim(uint64_t* freed_bytes) {
    if (!k2r::Runtime::get().ok) return DCDF_ERR_NO_DEVICE;
    (void)hipDeviceSynchronize();
    const size_t f = k2r::DevPool::get().drain();
    if (freed_bytes) *freed_bytes = (uint64_t)f;
    return DCDF_OK;
}
extern "C" int dcdf_last_hip_error(void) { return k2r::last_hip_error(); }
