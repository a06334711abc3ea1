/*
 * kernel_cl_shim.h — the whole of the OpenCL device runtime that the reference's kernel.cl uses, for a CPU
 * build of that file as plain C (gcc -x c -include kernel_cl_shim.h). TEST INFRASTRUCTURE ONLY.
 *
 * kernel.cl is C apart from two qualifiers and two work-item queries. The qualifiers expand to nothing; the
 * queries read the position that kernel_cl_driver.c sets before it calls a kernel for one work-item.
 * Nothing here is taken from the reference.
 */
#ifndef KERNEL_CL_SHIM_H
#define KERNEL_CL_SHIM_H

#define __kernel
#define __global

extern _Thread_local int kcl_global_id[2];
extern _Thread_local int kcl_global_size[2];

static inline int get_global_id(int d) { return kcl_global_id[d]; }
static inline int get_global_size(int d) { return kcl_global_size[d]; }

#endif
