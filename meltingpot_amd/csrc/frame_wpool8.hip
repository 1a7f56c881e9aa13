// frame_wpool8.hip — WORLD.RGB pooled by 8 (frame_wpool.h)
#define MP_WPOOL 8
#include "frame_wpool.h"
