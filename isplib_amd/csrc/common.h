// common.h -- error plumbing shared by the HIP translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "../../include/isplib_hip.h"

namespace isplib {

char *error_buffer();   // thread-local, 512 bytes (defined in runtime.hip)
int empty_row_init();   // 1: an empty row of max / min keeps the reference launcher's pre-fill (isplib_hip_set_empty_row; runtime.hip)

int stream_stage_mode();                     // ISPLIB_STAGE_*: staged column panels of the stream schedule (ISPLIB_STREAM_STAGE; runtime.hip)
void stream_stage_report(unsigned panels);   // which panels the call staged (isplib_stream_stage_last)
// mean loop ticks of every wave of one generation of the sum / mean stream kernel on a synthetic plan (spmm_sweep.hip): the calibration
// behind isplib_stream_capacities_hip (stream_plan.hip); `launches` timed launches after one that is not counted
int stream_kernel_calibrate(int streams, int waves_per_gen, int launches, int degree, int col_mult, double *wave_ticks, hipStream_t st);
// the packed word stream of the sum / mean stream kernel (ISPLIB_STREAM_PACK; runtime.hip)
enum { ISPLIB_PACK_OFF = 0, ISPLIB_PACK_FORCE = 1, ISPLIB_PACK_AUTO = 2 };
int stream_pack_mode();
void stream_pack_report(int packed);         // whether the call launched the PACKED instance (isplib_stream_pack_last)
int stream_level_mode();                     // 0 off, 1 on, 2 auto: the levelled deal of the stream plans (ISPLIB_STREAM_LEVEL; runtime.hip)

inline void clear_error() { error_buffer()[0] = '\0'; }

inline int fail(int code, const char *msg) {
   snprintf(error_buffer(), 512, "%s", msg);
   return code;
}

inline int fail(int code, const char *entry, const char *msg) {      // "<entry>: <msg>"
   snprintf(error_buffer(), 512, "%s: %s", entry, msg);
   return code;
}

inline int hip_fail(hipError_t e, const char *what) {
   snprintf(error_buffer(), 512, "%s: %s", what, hipGetErrorString(e));
   return ISPLIB_HIP_ERROR;
}

// (out of line: one copy per library, not one per launch site)
__attribute__((noinline)) inline int check_launch(const char *what) {
   const hipError_t e = hipGetLastError();
   return e == hipSuccess ? ISPLIB_SUCCESS : hip_fail(e, what);
}

#define ISPLIB_HIP_TRY(expr)                                        \
   do {                                                             \
      const hipError_t e_ = (expr);                                 \
      if (e_ != hipSuccess) return ::isplib::hip_fail(e_, #expr);   \
   } while (0)

}  // namespace isplib
