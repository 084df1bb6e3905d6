// rmav_rollout_rung.inc - rmav_rollout_body.inc with the guards of a wrapper above the disturbance rung.  The wrapper says how far up the
// feature ladder it is - #define RMAV_RUNG 5 (*_sn), 6 (*_al), 7 (*_ss) or 8 (*_tc): the numbers of rmav_ladder.hpp's enum - and
// includes this file.  Every guard of a rung at or below that number is on while the body is compiled; behind it every guard is 0 again
// and RMAV_RUNG is gone, so no wrapper can change a kernel defined below it.
#if !defined(RMAV_RUNG) || RMAV_RUNG < 5 || RMAV_RUNG > 8
#error "rmav_rollout_rung.inc: #define RMAV_RUNG 5 .. 8 in front of the #include"
#endif
#undef RMAV_ROLLOUT_SN
#undef RMAV_ROLLOUT_AL
#undef RMAV_ROLLOUT_SS
#undef RMAV_ROLLOUT_TC
#define RMAV_ROLLOUT_SN (RMAV_RUNG >= 5)
#define RMAV_ROLLOUT_AL (RMAV_RUNG >= 6)
#define RMAV_ROLLOUT_SS (RMAV_RUNG >= 7)
#define RMAV_ROLLOUT_TC (RMAV_RUNG >= 8)
#include "rmav_rollout_body.inc"
#undef RMAV_ROLLOUT_SN
#undef RMAV_ROLLOUT_AL
#undef RMAV_ROLLOUT_SS
#undef RMAV_ROLLOUT_TC
#define RMAV_ROLLOUT_SN 0
#define RMAV_ROLLOUT_AL 0
#define RMAV_ROLLOUT_SS 0
#define RMAV_ROLLOUT_TC 0
#undef RMAV_RUNG
