// frame_wpool4.hip — WORLD.RGB pooled by 4 (frame_wpool.h)
#define MP_WPOOL 4
#include "frame_wpool.h"
