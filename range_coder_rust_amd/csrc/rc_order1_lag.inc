// rc_order1_lag.inc — one translation unit of the lagged order-1 coders (DESIGN.md §9.15): the
// kernels of rc_order1.inc instantiated with O1MapLag<RC_O1_LAG> and their launchers.  Included by
// rc_order1_lag{2,4,8}.hip, which define RC_O1_LAG: a unit per lag keeps the lag-1 unit
// (rc_order1.hip) as it was and lets the four build side by side.
#ifndef RC_O1_LAG
#error "define RC_O1_LAG (2, 4 or 8) before including rc_order1_lag.inc"
#endif
#include "rc_order1.inc"

template <>
hipError_t rc_order1_encode_launch_lag<RC_O1_LAG>(hipStream_t stream, const RcKnobs& k,
                                                  const O1Args& a_in, int div, const SetPlan& p,
                                                  const uint8_t* syms, const u64* sym_off,
                                                  u32 n_chunks, uint8_t* out, const u64* out_off,
                                                  u64* out_len, u32* flags) {
  using MAP = O1MapLag<RC_O1_LAG>;
  O1Args a = a_in;
  a.s.tab_bytes = p.enc_tab;
  auto go = [&](auto kern) {
    return cuwg_launch(kern, stream, k, a, a.s.m, kPrioEncoder, p.enc_lanes, SET_ENC_LANE_BYTES,
                       p.enc_lds, n_chunks, syms, sym_off, n_chunks, out, out_off, out_len, flags);
  };
  if (div == DIV_POW2)
    return p.enc_layout == 0 ? go(k_encode_order1<DIV_POW2, 0, MAP>)
                             : go(k_encode_order1<DIV_POW2, 1, MAP>);
  return p.enc_layout == 0 ? go(k_encode_order1<DIV_MAGIC, 0, MAP>)
                           : go(k_encode_order1<DIV_MAGIC, 1, MAP>);
}

template <>
hipError_t rc_order1_decode_launch_lag<RC_O1_LAG>(hipStream_t stream, const RcKnobs& k,
                                                  const O1Args& a_in, int div, const SetPlan& p,
                                                  const uint8_t* code, const u64* code_off,
                                                  const u64* code_len, uint8_t* syms_out,
                                                  const u64* sym_off, u32 n_chunks, u32* flags) {
  using MAP = O1MapLag<RC_O1_LAG>;
  O1Args a = a_in;
  auto go = [&](auto kern) {
    return cuwg_launch(kern, stream, k, a, a.s.m, kPrioDecoder512, p.dec_lanes,
                       SET_DEC_LANE_BYTES, p.dec_lds, n_chunks, code, code_off, code_len, syms_out,
                       sym_off, n_chunks, flags);
  };
  return div == DIV_POW2 ? go(k_decode_order1<DIV_POW2, MAP>)
                         : go(k_decode_order1<DIV_MAGIC, MAP>);
}
