// rmav_pair_rung.inc - a pair body with the guards of a wrapper on the feature ladder.  The wrapper says how far up it is -
// #define RMAV_RUNG 1 (*_dr), 2 (*_fs), 3 (*_rw), 4 (*_ds), 5 (*_sn), 6 (*_al), 7 (*_ss) or 8 (*_tc): the numbers of rmav_ladder.hpp's enum -
// names its body - #define RMAV_PAIR_BODY "rmav_pair_body.inc" or "rmav_pair_shared_body.inc" - and includes this file.  Every guard of a
// rung at or below that number is on while the body is compiled (the skip and the reward have none: their bodies are the ranged one's);
// behind it every guard is 0 again and both names are gone, so no wrapper can change a kernel defined below it.
#if !defined(RMAV_RUNG) || !defined(RMAV_PAIR_BODY) || RMAV_RUNG < 1 || RMAV_RUNG > 8
#error "rmav_pair_rung.inc: #define RMAV_RUNG 1 .. 8 and RMAV_PAIR_BODY in front of the #include"
#endif
#undef RMAV_PAIR_DR
#undef RMAV_PAIR_DS
#undef RMAV_PAIR_SN
#undef RMAV_PAIR_AL
#undef RMAV_PAIR_SS
#undef RMAV_PAIR_TC
#define RMAV_PAIR_DR (RMAV_RUNG >= 1)
#define RMAV_PAIR_DS (RMAV_RUNG >= 4)
#define RMAV_PAIR_SN (RMAV_RUNG >= 5)
#define RMAV_PAIR_AL (RMAV_RUNG >= 6)
#define RMAV_PAIR_SS (RMAV_RUNG >= 7)
#define RMAV_PAIR_TC (RMAV_RUNG >= 8)
#include RMAV_PAIR_BODY
#undef RMAV_PAIR_DR
#undef RMAV_PAIR_DS
#undef RMAV_PAIR_SN
#undef RMAV_PAIR_AL
#undef RMAV_PAIR_SS
#undef RMAV_PAIR_TC
#define RMAV_PAIR_DR 0
#define RMAV_PAIR_DS 0
#define RMAV_PAIR_SN 0
#define RMAV_PAIR_AL 0
#define RMAV_PAIR_SS 0
#define RMAV_PAIR_TC 0
#undef RMAV_RUNG
#undef RMAV_PAIR_BODY
