// rc_order1_lag8.hip — the order-1 coders at a lag of 8 symbols (rc_order1_lag.inc).
#define RC_O1_LAG 8
#include "rc_order1_lag.inc"
