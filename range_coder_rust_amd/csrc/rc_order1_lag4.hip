// rc_order1_lag4.hip — the order-1 coders at a lag of 4 symbols (rc_order1_lag.inc).
#define RC_O1_LAG 4
#include "rc_order1_lag.inc"
