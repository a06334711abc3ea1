/*
 * mbn_panoptic.c — the host side of "score a segmentation by its regions" (include/mbn.h): what mbn_panoptic_i32 accepts, the scratch a handle
 * holds and the metrics of a pq table. Pure C, no HIP: libmbn_host.so carries it.
 */
#include <math.h>
#include <stddef.h>

#include "mbn.h"
#include "mbn_envelope.h"

int mbn_panoptic_envelope(int batch, int rows, int cols, int classes, int max_pred, int max_truth)
{
    if (batch < 1 || rows < 1 || cols < 1 || classes < 1 || max_pred < 1 || max_truth < 1) return MBN_EINVAL;
    /* areas are int32 and inter * 2^32 must fit a uint64: a map stays below 2^29 pixels; a truth number has MBN_PANOPTIC_BITS bits */
    if ((int64_t)rows * cols >= MBN_COMPONENTS_MAX_MAP || batch > MBN_DENSE_MAX_BATCH || max_pred > MBN_COMPONENTS_MAX_REGIONS ||
        max_truth > MBN_COMPONENTS_MAX_REGIONS || classes > MBN_CONFUSION_MAX_CLASSES)
        return MBN_EUNSUPPORTED;
    return MBN_OK;
}

/* MBN_PANOPTIC_SLOT_WORDS + 1 int32 per predicted slot (its counters and its candidate) and one per truth slot. Rounded up to 256 bytes. 0 for arguments mbn_panoptic_create refuses */
int64_t mbn_panoptic_scratch_bytes(int max_batch, int64_t max_slots)
{
    if (max_batch < 1 || max_slots < 1 || max_batch > MBN_DENSE_MAX_BATCH || max_slots > MBN_PANOPTIC_MAX_SLOTS) return 0;
    const int64_t bytes = 4 * (MBN_PANOPTIC_SLOT_WORDS + 2) * max_slots;
    return (bytes + 255) / 256 * 256;
}

int mbn_panoptic_metrics(const uint64_t *pq, int classes, mbn_panoptic_metrics_t *m, double *pq_c, double *sq_c, double *rq_c)
{
    if (!pq || !m || classes < 1) return MBN_EINVAL;
    if (classes > MBN_CONFUSION_MAX_CLASSES) return MBN_EUNSUPPORTED;
    double pq_sum = 0.0, sq_sum = 0.0, rq_sum = 0.0, tp_sum = 0.0, fp_sum = 0.0, fn_sum = 0.0;
    int present = 0;
    for (int c = 0; c < classes; c++) {
        const double tp = (double)pq[4 * (size_t)c], fp = (double)pq[4 * (size_t)c + 1], fn = (double)pq[4 * (size_t)c + 2];
        const double iou = ldexp((double)pq[4 * (size_t)c + 3], -32);
        const double den = 2.0 * tp + fp + fn;
        double p = (double)NAN, s = (double)NAN, r = (double)NAN;
        if (tp + fp + fn > 0.0) {
            p = 2.0 * iou / den;                                     /* the doublings are exact: each value is one division */
            r = 2.0 * tp / den;
            s = tp > 0.0 ? iou / tp : 0.0;
            present++;
            pq_sum += p; sq_sum += s; rq_sum += r;
        }
        if (pq_c) pq_c[c] = p;
        if (sq_c) sq_c[c] = s;
        if (rq_c) rq_c[c] = r;
        tp_sum += tp; fp_sum += fp; fn_sum += fn;
    }
    m->pq = present ? pq_sum / (double)present : 0.0;
    m->sq = present ? sq_sum / (double)present : 0.0;
    m->rq = present ? rq_sum / (double)present : 0.0;
    m->tp = tp_sum; m->fp = fp_sum; m->fn = fn_sum;
    m->classes_present = present;
    m->reserved = 0;
    return MBN_OK;
}
