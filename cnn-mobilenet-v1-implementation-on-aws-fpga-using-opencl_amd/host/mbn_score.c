/*
 * mbn_score.c — the host side of "score a segmentation" (include/mbn.h): what mbn_confusion_i32 accepts, which form of the kernel a class count
 * takes, and the standard metrics of a confusion matrix; the same for the rank score and the calibration score. Pure C, no HIP: libmbn_host.so
 * carries it.
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

/* ---- calibration score (include/mbn.h, "calibration score"): what mbn_calibration_f32 accepts, and the reliability diagram, the expected
 * calibration error and the risk-coverage curve of a table */
int mbn_calibration_envelope(int classes, int truth_bytes, int bins, int64_t count)
{
    const int shape = mbn_confusion_envelope(classes, truth_bytes, count);
    if (bins < 1 || shape == MBN_EINVAL) return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    return bins > MBN_CALIBRATION_MAX_BINS ? MBN_EUNSUPPORTED : MBN_OK;
}

static int calibration_table_check(const uint64_t *calib, int bins)
{
    if (!calib || bins < 1) return MBN_EINVAL;
    return bins > MBN_CALIBRATION_MAX_BINS ? MBN_EUNSUPPORTED : MBN_OK;
}

/* cell (b, col) as a double: exact below 2^53 */
static double calibration_cell(const uint64_t *calib, int b, int col) { return (double)calib[(size_t)b * 4 + (size_t)col]; }

int mbn_calibration_metrics(const uint64_t *calib, int bins, mbn_calibration *m, double *accuracy, double *confidence, double *coverage,
                            double *selective_accuracy)
{
    const int rc = calibration_table_check(calib, bins);
    if (rc != MBN_OK || !m) return rc != MBN_OK ? rc : MBN_EINVAL;
    const double one = 16777216.0;                                  /* 2^24: the fixed point of column 2 */
    /* sums of integers in doubles: exact below 2^53 */
    double answered = 0.0, right = 0.0, conf = 0.0, abstained = 0.0;
    for (int b = 0; b < bins; b++) {
        answered += calibration_cell(calib, b, 0);
        right += calibration_cell(calib, b, 1);
        conf += calibration_cell(calib, b, 2);
        abstained += calibration_cell(calib, b, 3);
    }
    double ece = 0.0, mce = 0.0;
    for (int b = 0; b < bins; b++) {                                /* ascending bin order */
        const double n = calibration_cell(calib, b, 0);
        const double acc = n > 0.0 ? calibration_cell(calib, b, 1) / n : (double)NAN;
        const double cf = n > 0.0 ? calibration_cell(calib, b, 2) / (n * one) : (double)NAN;
        if (accuracy) accuracy[b] = acc;
        if (confidence) confidence[b] = cf;
        if (n > 0.0) {
            const double gap = fabs(acc - cf);
            ece += (n / answered) * gap;
            if (gap > mce) mce = gap;
        }
    }
    /* the curve of keeping the bins >= j, from the last edge down; aurc sums its terms in ascending j, so they are kept first */
    const double asked = answered + abstained;
    double kept = 0.0, kept_right = 0.0, aurc = 0.0, next = 0.0;
    double term[MBN_CALIBRATION_MAX_BINS];
    for (int j = bins - 1; j >= 0; j--) {
        kept += calibration_cell(calib, j, 0);
        kept_right += calibration_cell(calib, j, 1);
        const double cov = asked > 0.0 ? kept / asked : 0.0;
        const double sel = kept > 0.0 ? kept_right / kept : (double)NAN;
        if (coverage) coverage[j] = cov;
        if (selective_accuracy) selective_accuracy[j] = sel;
        term[j] = kept > 0.0 ? (1.0 - sel) * (cov - next) : 0.0;    /* an empty term is skipped */
        next = cov;
    }
    for (int j = 0; j < bins; j++) aurc += term[j];
    m->answered = answered;
    m->abstained = abstained;
    m->void_pixels = calibration_cell(calib, bins, 0);
    m->pixels = answered + abstained + m->void_pixels;
    m->accuracy = answered > 0.0 ? right / answered : 0.0;
    m->mean_confidence = answered > 0.0 ? conf / (answered * one) : 0.0;
    m->ece = ece;
    m->mce = mce;
    m->aurc = aurc;
    return MBN_OK;
}

int mbn_calibration_threshold(const uint64_t *calib, int bins, double target_accuracy, float *min_prob, double *coverage,
                              double *selective_accuracy)
{
    const int rc = calibration_table_check(calib, bins);
    if (rc != MBN_OK) return rc;
    if (!(target_accuracy >= 0.0 && target_accuracy <= 1.0)) return MBN_EINVAL;
    double answered = 0.0, abstained = 0.0, right = 0.0;
    for (int b = 0; b < bins; b++) {
        answered += calibration_cell(calib, b, 0);
        right += calibration_cell(calib, b, 1);
        abstained += calibration_cell(calib, b, 3);
    }
    /* kept / kept_right at edge j are the sums over b >= j: the totals less the bins in front, exact integers */
    double kept = answered, kept_right = right;
    for (int j = 0; j < bins; j++) {
        if (kept > 0.0 && kept_right / kept >= target_accuracy) {
            if (min_prob) *min_prob = (float)j / (float)bins;
            if (coverage) *coverage = kept / (answered + abstained);
            if (selective_accuracy) *selective_accuracy = kept_right / kept;
            return MBN_OK;
        }
        kept -= calibration_cell(calib, j, 0);
        kept_right -= calibration_cell(calib, j, 1);
    }
    return MBN_ENOTFOUND;
}

/* ---- score the probabilities (include/mbn.h, "score the probabilities"): the NLL, the Brier score and the accuracy of one temperature plane of
 * the table mbn_resample_nll_f32 adds to, and the plane of a temperature grid with the smallest NLL */
static int nll_table_check(const uint64_t *nll_u64, int classes, int temps)
{
    if (!nll_u64 || classes < 1 || temps < 1 || temps > MBN_NLL_MAX_TEMPS) return MBN_EINVAL;
    return classes > MBN_CONFUSION_MAX_CLASSES ? MBN_EUNSUPPORTED : MBN_OK;
}

/* cell (t, col) of plane j as a double: exact below 2^53 */
static double nll_cell(const uint64_t *nll_u64, int classes, int j, int t, int col)
{
    return (double)nll_u64[((size_t)j * ((size_t)classes + 1) + (size_t)t) * 4 + (size_t)col];
}

int mbn_nll_metrics(const uint64_t *nll_u64, int classes, int temps, int j, mbn_nll *m, double *class_nll, double *class_brier)
{
    const int rc = nll_table_check(nll_u64, classes, temps);
    if (rc == MBN_EINVAL || !m || j < 0 || j >= temps) return MBN_EINVAL;
    if (rc != MBN_OK) return rc;
    const double one16 = 65536.0, one24 = 16777216.0;               /* the fixed points of columns 1 and 2 */
    /* sums of integers in doubles: exact below 2^53 */
    double scored = 0.0, nll = 0.0, brier = 0.0, right = 0.0, mean_nll = 0.0, mean_brier = 0.0;
    int present = 0;
    for (int t = 0; t < classes; t++) {                             /* ascending class order */
        const double n = nll_cell(nll_u64, classes, j, t, 0), a = nll_cell(nll_u64, classes, j, t, 1), b = nll_cell(nll_u64, classes, j, t, 2);
        scored += n; nll += a; brier += b;
        right += nll_cell(nll_u64, classes, j, t, 3);
        const double cn = n > 0.0 ? a / (n * one16) : (double)NAN, cb = n > 0.0 ? b / (n * one24) : (double)NAN;
        if (class_nll) class_nll[t] = cn;
        if (class_brier) class_brier[t] = cb;
        if (n > 0.0) { present++; mean_nll += cn; mean_brier += cb; }
    }
    m->scored = scored;
    m->void_pixels = nll_cell(nll_u64, classes, j, classes, 0);
    m->pixels = scored + m->void_pixels;
    m->nll = scored > 0.0 ? nll / (scored * one16) : 0.0;
    m->brier = scored > 0.0 ? brier / (scored * one24) : 0.0;
    m->accuracy = scored > 0.0 ? right / scored : 0.0;
    m->mean_class_nll = present ? mean_nll / (double)present : 0.0;
    m->mean_class_brier = present ? mean_brier / (double)present : 0.0;
    m->classes_present = present;
    return MBN_OK;
}

int mbn_nll_best(const uint64_t *nll_u64, int classes, int temps, const float *inv_temps, int *best, double *inv_temp, int *at_edge)
{
    const int rc = nll_table_check(nll_u64, classes, temps);
    if (rc == MBN_EINVAL || !inv_temps || !best) return MBN_EINVAL;
    for (int j = 0; j < temps; j++)
        if (!(inv_temps[j] > 0.0f) || isinf(inv_temps[j]) || (j > 0 && !(inv_temps[j] > inv_temps[j - 1]))) return MBN_EINVAL;
    if (rc != MBN_OK) return rc;
    /* the integer sums of column 1 (they fit: the device's 64-bit cells did), and what plane 0 scored */
    uint64_t sum[MBN_NLL_MAX_TEMPS], scored = 0;
    for (int t = 0; t < classes; t++) scored += nll_u64[(size_t)t * 4];
    if (!scored) return MBN_ENOTFOUND;
    int b = 0;
    for (int j = 0; j < temps; j++) {
        sum[j] = 0;
        for (int t = 0; t < classes; t++) sum[j] += nll_u64[((size_t)j * ((size_t)classes + 1) + (size_t)t) * 4 + 1];
        if (sum[j] < sum[b]) b = j;                                 /* strict: the lowest index on a tie */
    }
    double beta = (double)inv_temps[b];
    if (b > 0 && b + 1 < temps) {
        const double x0 = log((double)inv_temps[b - 1]), x1 = log((double)inv_temps[b]), x2 = log((double)inv_temps[b + 1]);
        const double y0 = (double)sum[b - 1], y1 = (double)sum[b], y2 = (double)sum[b + 1];
        const double s01 = (y1 - y0) / (x1 - x0), s12 = (y2 - y1) / (x2 - x1), a = (s12 - s01) / (x2 - x0);
        if (a > 0.0) {
            double x = 0.5 * (x0 + x1) - s01 / (2.0 * a);
            if (x < x0) x = x0;
            if (x > x2) x = x2;
            beta = exp(x);
        }
    }
    *best = b;
    if (inv_temp) *inv_temp = beta;
    if (at_edge) *at_edge = temps > 1 && (b == 0 || b == temps - 1);
    return MBN_OK;
}
