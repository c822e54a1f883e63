// rc_host.h — the library's one internal host header: the context, the model,
// the device guard, and the one declaration of every function that one translation unit defines
// and another calls.  Every unit that takes an rc_ctx or an rc_model includes it and reads the
// fields; no .hip or .inc file writes a prototype of its own.  The family launchers are declared
// by the family headers included here; so are the two launch helpers that the kernel units call
// as well (rc_resident_wgs and set_allow_lds: rc_static.h).
#pragma once
#include "rc_static.h"
#include "rc_indexed.h"
#include "rc_order1.h"
#include "rc_wide.h"
#include "rc_wide16.h"
#include "rc_wide16_fine.h"
#include "rc_chunk_set.h"

struct rc_ctx {
  int device;
  hipStream_t own;
  hipStream_t cur;
  uint8_t* inv;  // 64 KiB device scratch for rc_synth_fill's inverse CDF
  RcKnobs knobs;  // read from the environment once, by rc_ctx_create (rc_common.h)
  // rc_rows.hip only: rc_stream_decode_rows's decoder (rc_rows_decoder_: 0 by the rule, 1 wave,
  // 2 lane) and the device's CU count for the rule (0: not asked yet)
  u32 rows_decoder = 0;
  u32 n_cus = 0;
  GroupScratch group;  // the chunk-set calls' grouping scratch (rc_chunk_set.h), grown on demand
};

enum {
  RC_KIND_STATIC = 0,
  RC_KIND_ADAPTIVE = 1,
  RC_KIND_SET = 2,
  RC_KIND_WIDE = 3,
  RC_KIND_ORDER1 = 4,
  RC_KIND_CHUNK_SET = 5,
  RC_KIND_WIDE16 = 6
};

struct rc_model {
  int kind;  // 0 static, 1 adaptive, 2 static model set (rc_indexed.h: `set` and `plan`),
             // 3 wide static model (rc_wide.h: `wide` and `wplan`), 4 order-1 set (rc_order1.h:
             // `o1` and `plan`)
  SetArgs set;
  SetPlan plan;
  WideArgs wide;
  WidePlan wplan;
  Wide16Args w16;  // kind 6, a wide16 static model (rc_wide16.h): `w16` and `w16plan`
  Wide16Plan w16plan;
  Wide16FineArgs w16f;  // kind 6 with w16_fine: a wide16 fine model (rc_wide16_fine.h): `w16f` and
  bool w16_fine;        // `w16plan`; the wide16 batch calls launch its kernels
  ChunkSetArgs cset;  // kind 5, a static chunk set (rc_chunk_set.h): `args` is row 0's
  O1Args o1;  // kind 4 (o1.period: 1, 2, 4 or 8)
  u32 o1_lag;  // kind 4: 1, 2, 4 or 8 (rc_order1.h: no field of the kernels' O1Args)
  int device;
  int div;
  ModelArgs args;
  void* dmem;
  AdaptParams ap;      // kind 1
  u32 c_host[256];     // kind 0: the c_freq snapshot (container tables, entropy reports)
  u32 period;          // kind 1: as given
  bool complete;       // kind 0: 256 symbols, every c_freq > 0 (no symbol the coder can reject)
};

// Kinds do not mix: an entry point names the kinds it accepts, as bits 1 << kind, and refuses
// every other model (RC_E_ARG), a kind added later included.
// (RC_KINDS_SINGLE: the models of one table over one-byte symbols)
static const u32 RC_KINDS_SINGLE = 1u << RC_KIND_STATIC | 1u << RC_KIND_ADAPTIVE;
static inline bool rc_model_kind_ok(const rc_model* m, u32 kinds) {
  return m && ((kinds >> m->kind) & 1u);
}

// The calling thread's current device set to `dev` until the end of the scope.  ok: the device
// could be set (a caller that went on regardless before this header still may).  (Unnamed
// namespace: every unit compiles its own copy, and the library exports none.)
namespace {
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    int now = -1;
    if (prev >= 0 && hipGetDevice(&now) == hipSuccess && now != prev) (void)hipSetDevice(prev);
  }
};
}  // namespace

// rc_kernels.hip.  A pinned host buffer of at least `bytes` (<= 1 MiB) for this host thread,
// grown on demand.  Host <-> device transfers of small control data go through it: async copies
// to and from pageable memory returned wrong bytes intermittently on this stack,
// pinned ones are plain stream-ordered DMA.  Contents are the caller's until its next call on the
// same thread.
void* rc_pinned_scratch_(size_t bytes);
// rc_kernels.hip: the run-time switches as the environment gives them (rc_ctx_create only)
RcKnobs rc_knobs_from_env();
// rc_resume.hip: ask the process's stream-service waves to leave before a batch launch (a
// resident wave would hold the hardware queue its stream shares with the launch's)
void rc_svc_yield_all_();
extern "C" {
// rc_ctx_destroy's: free the context's cached host pipeline (rc_stream.hip) and the stream API's
// staging and service (rc_resume.hip)
void rc_stream_release_(const rc_ctx* ctx);
void rc_resume_release_(const rc_ctx* ctx);
}
