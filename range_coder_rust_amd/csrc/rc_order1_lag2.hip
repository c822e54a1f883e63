// rc_order1_lag2.hip — the order-1 coders at a lag of 2 symbols (rc_order1_lag.inc).
#define RC_O1_LAG 2
#include "rc_order1_lag.inc"
