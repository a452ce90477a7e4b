// runtime.hip -- version + thread-local error text of the C ABI.
#include <stdlib.h>
#include <string.h>

#include "common.h"

namespace isplib {
char *error_buffer() {
   static thread_local char buf[512] = {0};
   return buf;
}
}  // namespace isplib

// The one convention of the path that nothing in the reference tree pins: what an EMPTY row of a max / min
// SpMM holds.  The reference's launcher pre-fills the output with lowest() / max() and the positions with nnz
// (csrc/fusedmm.cpp:147-150,171,177) and hands both to fusedMM_csr, whose body is absent: a body that leaves untouched what it
// has no entry for returns -FLT_MAX / +FLT_MAX ("init"); torch_sparse's CPU kernel, the one the iSpLib authors compared with
// (isplib/__init__.py:120-128), writes 0 ("zero", the default here and in the oracle).  Process-wide: ISPLIB_EMPTY_ROW=init|zero
// read once, or isplib_hip_set_empty_row.  The positions are nnz either way; sum / mean are 0 either way.
namespace isplib {
static int g_empty_row = -1;
int empty_row_init() {
   if (g_empty_row < 0) {
      const char *e = getenv("ISPLIB_EMPTY_ROW");
      g_empty_row = (e && (strcmp(e, "init") == 0 || strcmp(e, "1") == 0)) ? 1 : 0;
   }
   return g_empty_row;
}
}  // namespace isplib

extern "C" int isplib_hip_set_empty_row(int init) {
   isplib::clear_error();
   if (init != 0 && init != 1) return isplib::fail(ISPLIB_FAIL, "isplib_hip_set_empty_row: 0 (zero) or 1 (the launcher's init value)");
   isplib::g_empty_row = init;
   return ISPLIB_SUCCESS;
}
extern "C" int isplib_hip_get_empty_row(void) { return isplib::empty_row_init(); }

// Staged column panels of the stream schedule (include/isplib_hip.h, isplib_stream_stage_panel): the process-wide mode,
// ISPLIB_STREAM_STAGE=auto|0|1 read once.  Unset: auto -- profiles/stream_stage_panels.txt holds the A/B that makes the rule the
// default (every staged run below every parent run, the median difference 40 spreads of the parent).  The two entries below are for A/B runs and tests and are not declared in the header:
// isplib_stream_stage_set overrides the mode (ISPLIB_STAGE_*), isplib_stream_stage_last reports which panels the last call of
// fusedMM_csr_stream_hip on this thread staged (bit p: panel p).
namespace isplib {
static int g_stream_stage = -1;
static thread_local unsigned g_stream_stage_last = 0;
int stream_stage_mode() {
   if (g_stream_stage < 0) {
      const char *e = getenv("ISPLIB_STREAM_STAGE");
      g_stream_stage = !e ? ISPLIB_STAGE_AUTO : strcmp(e, "0") == 0 ? ISPLIB_STAGE_OFF : strcmp(e, "1") == 0 ? ISPLIB_STAGE_FORCE : ISPLIB_STAGE_AUTO;
   }
   return g_stream_stage;
}
void stream_stage_report(unsigned panels) { g_stream_stage_last = panels; }
}  // namespace isplib

extern "C" int isplib_stream_stage_set(int mode) {
   isplib::clear_error();
   if (mode != ISPLIB_STAGE_OFF && mode != ISPLIB_STAGE_FORCE && mode != ISPLIB_STAGE_AUTO) return isplib::fail(ISPLIB_FAIL, "isplib_stream_stage_set: 0 (off), 1 (force) or 2 (auto)");
   isplib::g_stream_stage = mode;
   return ISPLIB_SUCCESS;
}
extern "C" unsigned isplib_stream_stage_last(void) { return isplib::g_stream_stage_last; }

// The levelled deal of the stream plans (include/isplib_hip.h, isplib_stream_capacities_hip): ISPLIB_STREAM_LEVEL=auto|0|1 read
// once; unset: auto (profiles/stream_level_ab.txt holds the A/B).  isplib_stream_level_set overrides it for A/B runs and tests
// (0 off, 1 on, 2 auto; not declared in the header).  0 gives the unlevelled plan, and with it the unlevelled launch, exactly.
namespace isplib {
static int g_stream_level = -1;
int stream_level_mode() {
   if (g_stream_level < 0) {
      const char *e = getenv("ISPLIB_STREAM_LEVEL");
      g_stream_level = !e ? 2 : strcmp(e, "0") == 0 ? 0 : strcmp(e, "1") == 0 ? 1 : 2;
   }
   return g_stream_level;
}
}  // namespace isplib

extern "C" int isplib_stream_level_set(int mode) {
   isplib::clear_error();
   if (mode < 0 || mode > 2) return isplib::fail(ISPLIB_FAIL, "isplib_stream_level_set: 0 (off), 1 (on) or 2 (auto)");
   isplib::g_stream_level = mode;
   return ISPLIB_SUCCESS;
}

// The packed word stream of the sum / mean stream kernel (include/isplib_hip.h, PACKED WORD STREAM): ISPLIB_STREAM_PACK=auto|0|1 read
// once; unset: auto (profiles/stream_packed_words.txt holds the A/B).  0 is the launch of a plan without a packed stream, exactly.  For
// A/B runs and tests, not declared in the header: isplib_stream_pack_set overrides the mode (0 off, 1 whenever the plan has a packed
// stream, 2 auto), isplib_stream_pack_last tells whether the last call of fusedMM_csr_stream_hip on this thread read the packed stream.
namespace isplib {
static int g_stream_pack = -1;
static thread_local int g_stream_pack_last = 0;
int stream_pack_mode() {
   if (g_stream_pack < 0) {
      const char *e = getenv("ISPLIB_STREAM_PACK");
      g_stream_pack = !e ? ISPLIB_PACK_AUTO : strcmp(e, "0") == 0 ? ISPLIB_PACK_OFF : strcmp(e, "1") == 0 ? ISPLIB_PACK_FORCE : ISPLIB_PACK_AUTO;
   }
   return g_stream_pack;
}
void stream_pack_report(int packed) { g_stream_pack_last = packed; }
}  // namespace isplib

extern "C" int isplib_stream_pack_set(int mode) {
   isplib::clear_error();
   if (mode != isplib::ISPLIB_PACK_OFF && mode != isplib::ISPLIB_PACK_FORCE && mode != isplib::ISPLIB_PACK_AUTO)
      return isplib::fail(ISPLIB_FAIL, "isplib_stream_pack_set: 0 (off), 1 (every plan that has a packed stream) or 2 (auto)");
   isplib::g_stream_pack = mode;
   return ISPLIB_SUCCESS;
}
extern "C" int isplib_stream_pack_last(void) { return isplib::g_stream_pack_last; }

extern "C" int isplib_hip_abi_version(void) { return ISPLIB_HIP_ABI_VERSION; }
extern "C" const char *isplib_hip_last_error(void) { return isplib::error_buffer(); }
