// rc_order1.hip — k_encode_order1 / k_decode_order1: the indexed coders (rc_indexed.hip) with the
// row of each symbol chosen by the chunk's previous symbol through a context map (order-1 sets,
// rc_order1.h).  Symbol i of a chunk is coded exactly as encoder.encode(&models[row_i], sym[i]) /
// decoder.decode(&models[row_i]), row_0 = first_row, row_i = ctx_map[sym[i-1]].  The arithmetic,
// both rings, the flush rounds, dec_apply and dec_rare are those of the single-table coders
// (rc_encode.inc, rc_decode.inc, rc_static.h); the rows, buckets and the launch shape are the
// set's.  There is no index stream: the encoder takes the previous symbol from its tile, the
// decoder carries the row from one decoded symbol to the next in a register.  Periodic sets
// (row_i = ctx_map[i mod P][sym[i-1]]) run the same kernels with another map policy.
// The device source is rc_order1.inc, which the units of the lagged sets share.
#include "rc_order1.inc"

// ------------------------------------------------------------------------------------------
// Host: the plan and the launchers
// ------------------------------------------------------------------------------------------
void rc_order1_plan(u32 K, u32 total, u32 period, SetPlan* p) {
  const u32 maps = period * O1_MAP_BYTES;
  if (period == 1) {
    // encoder: the set's plan as it is (the map takes the place of the poison row K, which both
    // layouts reserve at least O1_MAP_BYTES for)
    rc_set_plan(K, total, p);
    if (!p->enc_lanes) return;
  } else {
    memset(p, 0, sizeof *p);
    if (!o1_period_ok(period) || K < 1 || K > RC_MAX_SET_MODELS || total < 256 || total > 65536)
      return;
    // encoder: rc_set_plan's rule over K rows and P KiB of maps (no row K: the maps do not fit
    // it, and an order-1 set cannot reach it).  The lanes come out of the search again: at K = 8
    // the period-1 plan leaves 2 KiB of the CU free, so P = 4 already costs it a quarter of its
    // lanes.
    for (u32 lanes = 1024; lanes >= 256 && !p->enc_lanes; lanes -= 256) {
      const u32 rings = lanes * SET_ENC_LANE_BYTES;
      const u32 t8 = K * 2048u + maps;
      const u32 t4 = (K * 4u * SET_ROW_WORDS + maps + 1023u) & ~1023u;
      if (t8 + rings <= SET_LDS_BYTES) {
        p->enc_lanes = lanes;
        p->enc_layout = 0;
        p->enc_tab = t8;
      } else if (t4 + rings <= SET_LDS_BYTES) {
        p->enc_lanes = lanes;
        p->enc_layout = 1;
        p->enc_tab = t4;
      }
      p->enc_lds = p->enc_tab + rings;
    }
  }
  // decoder: rc_set_plan's rule with the maps counted beside the rows
  cuwg_dec_plan(p, total, K * 4u * SET_ROW_WORDS + maps, K, 8u);
}

// the launchers take the instantiation of the set's period: one map, or every slice staged; a
// lag of 2, 4 or 8 goes to the unit of that lag (rc_order1_lag.inc), which stages the slices
// whatever the period
#define O1_ENC_LAUNCH_ARGS \
  stream, k, a_in, div, p, syms, sym_off, n_chunks, out, out_off, out_len, flags
#define O1_DEC_LAUNCH_ARGS \
  stream, k, a_in, div, p, code, code_off, code_len, syms_out, sym_off, n_chunks, flags
hipError_t rc_order1_encode_launch(hipStream_t stream, const RcKnobs& k, const O1Args& a_in,
                                   u32 lag, int div, const SetPlan& p, const uint8_t* syms,
                                   const u64* sym_off, u32 n_chunks, uint8_t* out,
                                   const u64* out_off, u64* out_len, u32* flags) {
  if (lag == 2) return rc_order1_encode_launch_lag<2>(O1_ENC_LAUNCH_ARGS);
  if (lag == 4) return rc_order1_encode_launch_lag<4>(O1_ENC_LAUNCH_ARGS);
  if (lag == 8) return rc_order1_encode_launch_lag<8>(O1_ENC_LAUNCH_ARGS);
  O1Args a = a_in;
  a.s.tab_bytes = p.enc_tab;
  auto go = [&](auto kern) {
    return cuwg_launch(kern, stream, k, a, a.s.m, kPrioEncoder, p.enc_lanes, SET_ENC_LANE_BYTES,
                       p.enc_lds, n_chunks, syms, sym_off, n_chunks, out, out_off, out_len, flags);
  };
  auto pick = [&](auto map) {
    using MAP = decltype(map);
    if (div == DIV_POW2)
      return p.enc_layout == 0 ? go(k_encode_order1<DIV_POW2, 0, MAP>)
                               : go(k_encode_order1<DIV_POW2, 1, MAP>);
    return p.enc_layout == 0 ? go(k_encode_order1<DIV_MAGIC, 0, MAP>)
                             : go(k_encode_order1<DIV_MAGIC, 1, MAP>);
  };
  return a.period > 1 ? pick(O1MapP{}) : pick(O1Map1{});
}

hipError_t rc_order1_decode_launch(hipStream_t stream, const RcKnobs& k, const O1Args& a_in,
                                   u32 lag, int div, const SetPlan& p, const uint8_t* code,
                                   const u64* code_off, const u64* code_len, uint8_t* syms_out,
                                   const u64* sym_off, u32 n_chunks, u32* flags) {
  if (lag == 2) return rc_order1_decode_launch_lag<2>(O1_DEC_LAUNCH_ARGS);
  if (lag == 4) return rc_order1_decode_launch_lag<4>(O1_DEC_LAUNCH_ARGS);
  if (lag == 8) return rc_order1_decode_launch_lag<8>(O1_DEC_LAUNCH_ARGS);
  O1Args a = a_in;
  auto go = [&](auto kern) {
    return cuwg_launch(kern, stream, k, a, a.s.m, kPrioDecoder512, p.dec_lanes,
                       SET_DEC_LANE_BYTES, p.dec_lds, n_chunks, code, code_off, code_len, syms_out,
                       sym_off, n_chunks, flags);
  };
  auto pick = [&](auto map) {
    using MAP = decltype(map);
    return div == DIV_POW2 ? go(k_decode_order1<DIV_POW2, MAP>)
                           : go(k_decode_order1<DIV_MAGIC, MAP>);
  };
  return a.period > 1 ? pick(O1MapP{}) : pick(O1Map1{});
}
