/*
 * kernel_cl_driver.c — runs the reference's four OpenCL kernels, compiled for the CPU from kernel.cl itself
 * (see kernel_cl_shim.h and the Makefile's _ref/libkernel_cl.so), once per work-item of an emulated NDRange.
 * TEST INFRASTRUCTURE ONLY. Nothing here is taken from the reference: the four prototypes restate the
 * argument lists that the kernels are called with, and the rest is a loop.
 *
 * The kernels check no bounds. The caller (oracle/kernel_cl.py, oracle/ref_selftest.c) sizes every buffer
 * from the ref_max_* functions below, which give the largest element index a launch forms.
 */
#include <stddef.h>

_Thread_local int kcl_global_id[2];
_Thread_local int kcl_global_size[2];

void convolute(unsigned char *output, unsigned char *inp_image_r, unsigned char *inp_image_g,
               unsigned char *inp_image_b, int *filter_k, int rows, int cols, int filtersize, int stride,
               int op_size);
void depthwise(unsigned char *output, unsigned char *inp_image, int *filter_k, int rows, int cols,
               int filtersize, int stride, int op_size);
void pointwise(unsigned char *output, unsigned char *inp_image, int *filter_k, int rows, int cols,
               int filtersize, int op_size);
void pool(unsigned char *output, unsigned char *inp_image, int rows, int cols, int filtersize, int op_size);

/* Work-items in index order wi = ty * g0 + tx: order 0 ascending, 1 descending. A launch whose result
 * depends on the order has no defined result; the caller runs both and compares. */
#define FOR_EACH_WORK_ITEM(g0, g1, order, call)                                  \
    do {                                                                         \
        const long n_ = (long)(g0) * (g1);                                       \
        kcl_global_size[0] = (g0);                                               \
        kcl_global_size[1] = (g1);                                               \
        for (long k_ = 0; k_ < n_; k_++) {                                       \
            const long wi_ = (order) ? n_ - 1 - k_ : k_;                         \
            kcl_global_id[0] = (int)(wi_ % (g0));                                \
            kcl_global_id[1] = (int)(wi_ / (g0));                                \
            call;                                                                \
        }                                                                        \
    } while (0)

void ref_convolute(int g0, int g1, int order, unsigned char *output, unsigned char *inp_r, unsigned char *inp_g,
                   unsigned char *inp_b, int *filter_k, int rows, int cols, int filtersize, int stride, int op_size)
{
    FOR_EACH_WORK_ITEM(g0, g1, order,
                       convolute(output, inp_r, inp_g, inp_b, filter_k, rows, cols, filtersize, stride, op_size));
}

void ref_depthwise(int g0, int g1, int order, unsigned char *output, unsigned char *inp_image, int *filter_k,
                   int rows, int cols, int filtersize, int stride, int op_size)
{
    FOR_EACH_WORK_ITEM(g0, g1, order, depthwise(output, inp_image, filter_k, rows, cols, filtersize, stride, op_size));
}

void ref_pointwise(int g0, int g1, int order, unsigned char *output, unsigned char *inp_image, int *filter_k,
                   int rows, int cols, int filtersize, int op_size)
{
    FOR_EACH_WORK_ITEM(g0, g1, order, pointwise(output, inp_image, filter_k, rows, cols, filtersize, op_size));
}

void ref_pool(int g0, int g1, int order, unsigned char *output, unsigned char *inp_image, int rows, int cols,
              int filtersize, int op_size)
{
    FOR_EACH_WORK_ITEM(g0, g1, order, pool(output, inp_image, rows, cols, filtersize, op_size));
}

/* ------------------------------------------------------------------------------------------------------
 * The largest element index a launch forms, counted from the pointer handed in. -1: the arguments are not
 * ones this driver runs (non-positive sizes, or an index that does not fit the kernels' int arithmetic). */

static long fits_int(long v) { return v >= 0 && v <= 0x7fffffffL ? v : -1; }

/* convolute and depthwise read  in[yindex * g0 * stride + xindex * stride]  with yindex <= g1 - 1 + h and
 * xindex <= g0 - 1 + h, h = filtersize / 2 (negative yindex or xindex are not read). */
long ref_max_in_window(int g0, int g1, int filtersize, int stride)
{
    if (g0 <= 0 || g1 <= 0 || filtersize <= 0 || stride <= 0) return -1;
    const long h = filtersize / 2;
    return fits_int((g1 - 1 + h) * (long)g0 * stride + (g0 - 1 + h) * (long)stride);
}

/* taps one output channel consumes from filter_k: (2h + 1)^2 per input plane, so an even filtersize reads
 * the taps of the next odd one */
long ref_taps(int filtersize)
{
    const long h = filtersize / 2;
    return filtersize > 0 ? (2 * h + 1) * (2 * h + 1) : -1;
}

/* pointwise reads  in[(ty * g0 + tx) + rows * cols * i],  i < filtersize */
long ref_max_in_pointwise(int g0, int g1, int rows, int cols, int filtersize)
{
    if (g0 <= 0 || g1 <= 0 || rows <= 0 || cols <= 0 || filtersize <= 0) return -1;
    return fits_int((long)rows * cols * (filtersize - 1) + (long)g0 * g1 - 1);
}

/* pool reads  in[i + rows * cols * c],  i < filtersize^2, c < op_size */
long ref_max_in_pool(int rows, int cols, int filtersize, int op_size)
{
    if (rows <= 0 || cols <= 0 || filtersize <= 0 || op_size <= 0) return -1;
    return fits_int((long)rows * cols * (op_size - 1) + (long)filtersize * filtersize - 1);
}

/* every kernel writes  out[(ty * g0 + tx) + shift * c],  c < op_size; shift is (rows / 2) * (cols / 2) for
 * convolute, rows * cols for depthwise and pointwise, 1 for pool */
long ref_max_out(int g0, int g1, long shift, int op_size)
{
    if (g0 <= 0 || g1 <= 0 || shift < 0 || op_size <= 0) return -1;
    return fits_int((long)g0 * g1 - 1 + shift * (op_size - 1));
}
