// bsx_align_ah.hip — the emitting twins of the two kernels that finish units, k_align_ah and k_hctrl_ah (all hits: include/bsx.h), and their
// launchers.  The device code is bsx_align.hip's own, compiled a second time with the all-hits emission behind unit_finish; it lives in a translation unit of
// its own so that the kernels of bsx_align.hip stay exactly what they are without it.
#define BSX_ALL_HITS_TU 1
#include "bsx_align.hip"
