/*
 * mbn_score.c — the host side of "score a segmentation" (include/mbn.h): what mbn_confusion_i32 accepts, which form of the kernel a class count
 * takes, and the standard metrics of a confusion matrix. Pure C, no HIP: libmbn_host.so carries it.
 */
#include <math.h>
#include <stddef.h>

#include "mbn.h"
#include "mbn_envelope.h"

int mbn_confusion_envelope(int classes, int truth_bytes, int64_t count)
{
    if (classes < 1 || count < 1 || (truth_bytes != 1 && truth_bytes != 4)) return MBN_EINVAL;
    if (classes > MBN_CONFUSION_MAX_CLASSES || count > MBN_CONFUSION_MAX_COUNT) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

/* one switch point: the table of (classes + 1)^2 32-bit bins fits MBN_CONFUSION_LDS up to MBN_CONFUSION_LDS_CLASSES */
int mbn_confusion_form(int classes)
{
    return classes <= MBN_CONFUSION_LDS_CLASSES ? MBN_CONFUSION_FORM_LDS : MBN_CONFUSION_FORM_GLOBAL;
}

int mbn_confusion_metrics(const uint64_t *counts, int classes, mbn_seg_metrics *m, double *iou)
{
    if (!counts || !m || classes < 1) return MBN_EINVAL;
    if (classes > MBN_CONFUSION_MAX_CLASSES) return MBN_EUNSUPPORTED;
    const size_t stride = (size_t)classes + 1;
    double valid = 0.0, void_pixels = 0.0, abstained = 0.0, tp_sum = 0.0;
    for (size_t col = 0; col < stride; col++) void_pixels += (double)counts[(size_t)classes * stride + col];
    /* the sums below are sums of integers in doubles: exact below 2^53 */
    double iou_sum = 0.0, acc_sum = 0.0, fw = 0.0;
    int present = 0, have_truth = 0;
    for (int t = 0; t < classes; t++) {
        double row = 0.0;
        for (size_t col = 0; col < stride; col++) row += (double)counts[(size_t)t * stride + col];
        valid += row;
        abstained += (double)counts[(size_t)t * stride + (size_t)classes];
        tp_sum += (double)counts[(size_t)t * stride + (size_t)t];
    }
    for (int c = 0; c < classes; c++) {
        double row = 0.0, fp = 0.0;
        for (size_t col = 0; col < stride; col++) row += (double)counts[(size_t)c * stride + col];
        for (int t = 0; t < classes; t++)
            if (t != c) fp += (double)counts[(size_t)t * stride + (size_t)c];
        const double tp = (double)counts[(size_t)c * stride + (size_t)c], fn = row - tp, den = tp + fp + fn;
        const double v = den > 0.0 ? tp / den : (double)NAN;
        if (iou) iou[c] = v;
        if (den > 0.0) {
            present++;
            iou_sum += v;
            fw += (row / valid) * v;                                /* den > 0 is made of cells of the valid rows: valid > 0 */
        }
        if (row > 0.0) {
            have_truth++;
            acc_sum += tp / row;
        }
    }
    m->pixels = valid + void_pixels;
    m->valid = valid;
    m->void_pixels = void_pixels;
    m->abstained = abstained;
    m->pixel_accuracy = valid > 0.0 ? tp_sum / valid : 0.0;
    m->mean_accuracy = have_truth ? acc_sum / (double)have_truth : 0.0;
    m->miou = present ? iou_sum / (double)present : 0.0;
    m->fw_iou = fw;
    m->classes_present = present;
    m->reserved = 0;
    return MBN_OK;
}

/* ---- rank score (include/mbn.h, "rank score"): what mbn_topk_rank_i32 accepts, which form of the kernel a table takes, and the top-1 .. top-k
 * accuracies of a rank table */
int mbn_topk_rank_envelope(int classes, int truth_bytes, int64_t count, int k, int64_t plane_stride)
{
    const int shape = mbn_confusion_envelope(classes, truth_bytes, count);
    if (k < 1 || k > MBN_TOPK_MAX || shape == MBN_EINVAL || plane_stride < count) return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    return plane_stride > MBN_TOPK_MAX_ELEMENTS / k ? MBN_EUNSUPPORTED : MBN_OK;
}

/* one switch point per k: the table of (classes + 1) * (k + 1) 32-bit bins fits MBN_TOPK_RANK_LDS */
int mbn_topk_rank_form(int classes, int k)
{
    return ((int64_t)classes + 1) * (k + 1) * 4 <= MBN_TOPK_RANK_LDS ? MBN_CONFUSION_FORM_LDS : MBN_CONFUSION_FORM_GLOBAL;
}

int mbn_topk_metrics(const uint64_t *ranks, int classes, int k, double *accuracy, double *mean_accuracy, double *valid)
{
    if (!ranks || classes < 1 || k < 1 || k > MBN_TOPK_MAX) return MBN_EINVAL;
    if (classes > MBN_CONFUSION_MAX_CLASSES) return MBN_EUNSUPPORTED;
    const size_t stride = (size_t)k + 1;
    /* sums of integers in doubles: exact below 2^53 */
    double hits[MBN_TOPK_MAX] = { 0.0 }, acc[MBN_TOPK_MAX] = { 0.0 }, total = 0.0;
    int have_truth = 0;
    for (int t = 0; t < classes; t++) {
        double row = 0.0, cum = 0.0;
        for (size_t col = 0; col < stride; col++) row += (double)ranks[(size_t)t * stride + col];
        total += row;
        if (row > 0.0) have_truth++;
        for (int j = 0; j < k; j++) {
            cum += (double)ranks[(size_t)t * stride + (size_t)j];
            hits[j] += cum;
            if (row > 0.0) acc[j] += cum / row;                  /* ascending class order */
        }
    }
    for (int j = 0; j < k; j++) {
        if (accuracy) accuracy[j] = total > 0.0 ? hits[j] / total : 0.0;
        if (mean_accuracy) mean_accuracy[j] = have_truth ? acc[j] / (double)have_truth : 0.0;
    }
    if (valid) *valid = total;
    return MBN_OK;
}
