// The library's error and ABI plumbing, host code only: the last-error text every entry point writes, the launch check, and the version /
// struct-size / device queries that ppmstereo_amd/_lib.py makes when it loads the library.
#include "common.h"

// ------------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
void ppms_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
int ppms_check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        ppms_set_error("%s: HIP launch failed: %s", what, hipGetErrorString(e));
        return PPMS_ELAUNCH;
    }
    return PPMS_OK;
}
extern "C" const char* ppms_last_error(void) { return g_err; }
extern "C" int ppms_version(void) { return PPMS_ABI_VERSION; }
extern "C" int ppms_struct_sizes(int* sp, int* epilogue, int* conv) {
    if (sp) *sp = (int)sizeof(ppms_sp);
    if (epilogue) *epilogue = (int)sizeof(ppms_epilogue);
    if (conv) *conv = (int)sizeof(ppms_conv);
    return PPMS_OK;
}
extern "C" int ppms_device_info(char* name, int name_cap, int* cu_count, int* clock_mhz) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        ppms_set_error("no HIP device");
        return PPMS_ENODEV;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        ppms_set_error("hipGetDeviceProperties failed");
        return PPMS_ENODEV;
    }
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", prop.gcnArchName);
    if (cu_count) *cu_count = prop.multiProcessorCount;
    if (clock_mhz) *clock_mhz = prop.clockRate / 1000;
    return PPMS_OK;
}
