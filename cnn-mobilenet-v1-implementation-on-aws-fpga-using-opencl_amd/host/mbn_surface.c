/*
 * mbn_surface.c — the host side of "score a segmentation by surface distance" (include/mbn.h): what the device calls accept, the unit of work
 * of their kernels, the scratch a handle holds, and Hausdorff distance, its percentile, ASSD and NSD of a surface table. Pure C, no HIP:
 * libmbn_host.so carries it.
 *
 * The table pools the contour pixels of every image and every call that added to it: each score here is a MICRO average over the dataset's
 * contour pixels (one long contour outweighs many short ones), not the mean of per-image scores.
 */
#include <math.h>
#include <stddef.h>

#include "mbn.h"
#include "mbn_envelope.h"

#define SURFACE_MAX_SIDE 32767                  /* 2 * 32766^2 < 2^31: a squared distance fits an int32 */
#define SURFACE_MAX_MAP ((int64_t)1 << 29)      /* indices inside a map are int32 */
#define SURFACE_MAX_PIXELS ((int64_t)1 << 34)   /* what one handle may hold */

int mbn_surface_envelope(int truth_bytes, int classes, int bins, int batch, int rows, int cols, int edge)
{
    if ((truth_bytes != 1 && truth_bytes != 4) || classes < 1 || bins < 2 || batch < 1 || rows < 1 || cols < 1 || (edge != 0 && edge != 1))
        return MBN_EINVAL;
    if (classes > MBN_CONFUSION_MAX_CLASSES || bins > MBN_SURFACE_MAX_BINS || rows > SURFACE_MAX_SIDE || cols > SURFACE_MAX_SIDE ||
        (int64_t)rows * cols >= SURFACE_MAX_MAP || batch > MBN_DENSE_MAX_BATCH)
        return MBN_EUNSUPPORTED;
    return MBN_OK;
}

int mbn_surface_tile(int *unit_pixels, int *wave_pixels)
{
    if (!unit_pixels || !wave_pixels) return MBN_EINVAL;
    *unit_pixels = MBN_SURFACE_UNIT;
    *wave_pixels = 64;
    return MBN_OK;
}

/* two int32 contour maps, and a presence word per side, image and class. Rounded up to 256 bytes. 0 for arguments mbn_surface_create refuses */
int64_t mbn_surface_scratch_bytes(int max_batch, int64_t max_pixels, int max_classes)
{
    if (max_batch < 1 || max_pixels < 1 || max_classes < 1 || max_batch > MBN_DENSE_MAX_BATCH || max_pixels > SURFACE_MAX_PIXELS ||
        max_classes > MBN_CONFUSION_MAX_CLASSES)
        return 0;
    const int64_t bytes = 8 * max_pixels + 8 * (int64_t)max_batch * max_classes;
    return (bytes + 255) / 256 * 256;
}

/* the smallest bin t whose cumulative count reaches `need` (need >= 1 and at most the sum of the bins) */
static int surface_reach(const uint64_t *bin, int bins, double need)
{
    double cum = 0.0;                           /* sums of integers in doubles: exact below 2^53 */
    for (int t = 0; t < bins - 1; t++) {
        cum += (double)bin[t];
        if (cum >= need) return t;
    }
    return bins - 1;
}

int mbn_surface_metrics(const uint64_t *surf, int classes, int bins, int tolerance, double percentile, mbn_surface_metrics_t *m, double *hd,
                        double *hdp, double *assd, double *nsd)
{
    if (!surf || !m || classes < 1 || bins < 2 || tolerance < 0 || tolerance > bins - 2 || !(percentile > 0.0 && percentile <= 100.0))
        return MBN_EINVAL;
    if (classes > MBN_CONFUSION_MAX_CLASSES || bins > MBN_SURFACE_MAX_BINS) return MBN_EUNSUPPORTED;
    const size_t stride = (size_t)MBN_SURFACE_HEAD + (size_t)bins;
    double sum_hd = 0.0, sum_hdp = 0.0, sum_assd = 0.0, sum_nsd = 0.0, total_n = 0.0, total_un = 0.0;
    int present = 0, measurable = 0, saturated = 0;
    for (int c = 0; c < classes; c++) {
        const uint64_t *row[2] = { surf + (size_t)c * 2 * stride, surf + ((size_t)c * 2 + 1) * stride };
        double n[2], matched[2], within[2];
        for (int k = 0; k < 2; k++) {
            n[k] = (double)row[k][0];
            matched[k] = n[k] - (double)row[k][1];
            within[k] = 0.0;
            for (int t = 0; t <= tolerance; t++) within[k] += (double)row[k][MBN_SURFACE_HEAD + t];
            total_n += n[k];
            total_un += (double)row[k][1];
        }
        double v_hd = (double)NAN, v_hdp = (double)NAN, v_assd = (double)NAN, v_nsd = (double)NAN;
        if (n[0] + n[1] > 0.0) {
            v_nsd = (within[0] + within[1]) / (n[0] + n[1]);
            present++;
            sum_nsd += v_nsd;
        }
        if (matched[0] > 0.0 && matched[1] > 0.0) {
            const uint64_t far = row[0][2] > row[1][2] ? row[0][2] : row[1][2];
            v_hd = sqrt((double)far);
            int t = 0;
            for (int k = 0; k < 2; k++) {
                const int tk = surface_reach(row[k] + MBN_SURFACE_HEAD, bins, ceil(percentile / 100.0 * matched[k]));
                if (tk > t) t = tk;
            }
            if (t == bins - 1) saturated++;
            v_hdp = (double)t;
            v_assd = ((double)row[0][3] + (double)row[1][3]) / 256.0 / (matched[0] + matched[1]);
            measurable++;
            sum_hd += v_hd; sum_hdp += v_hdp; sum_assd += v_assd;
        }
        if (hd) hd[c] = v_hd;
        if (hdp) hdp[c] = v_hdp;
        if (assd) assd[c] = v_assd;
        if (nsd) nsd[c] = v_nsd;
    }
    m->hd = measurable ? sum_hd / (double)measurable : 0.0;
    m->hdp = measurable ? sum_hdp / (double)measurable : 0.0;
    m->assd = measurable ? sum_assd / (double)measurable : 0.0;
    m->nsd = present ? sum_nsd / (double)present : 0.0;
    m->n = total_n;
    m->unmatched = total_un;
    m->classes_present = present;
    m->classes_measurable = measurable;
    m->saturated = saturated;
    m->reserved = 0;
    return MBN_OK;
}
