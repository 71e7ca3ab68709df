// pt_kernels_last.hip -- the light-only last bounce, k_bounce<false, MODE_LAST, FAST>, as a code object of its own at every
// arithmetic level.  The kernel IS pt_kernels.hip's k_bounce template -- same head, same pair tests, same deposit -- so this unit is that
// source with PT_KERNELS_LAST_UNIT: it instantiates that one mode, general and specialised, and exports its launcher as
// ptx_arith_last_<level>() (LastKernelSet, pt_kernels.h).  Compiled three times like pt_kernels.hip, with the same flags (Makefile).
#define PT_KERNELS_LAST_UNIT 1
#include "pt_kernels.hip"
