// frame_wpool2.hip — WORLD.RGB pooled by 2 (frame_wpool.h)
#define MP_WPOOL 2
#include "frame_wpool.h"
