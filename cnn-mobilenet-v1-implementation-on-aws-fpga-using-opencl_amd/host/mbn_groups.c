/*
 * mbn_groups.c — the host side of the group read-out (include/mbn.h, "segment by class groups"): the order in which the kernel walks the kept
 * classes. Plain C, no device call: part of libmbn_host.so.
 */
#include <stddef.h>

#include "mbn.h"

int mbn_class_groups_layout(int classes, int groups, const int32_t *group_of, int32_t *slot_class, int32_t *quad_group, int *slots)
{
    if (classes <= 0 || groups <= 0 || !group_of || !slot_class || !quad_group || !slots) return MBN_EINVAL;
    int kept = 0;
    for (int c = 0; c < classes; c++) {
        if (group_of[c] < -1 || group_of[c] >= groups) return MBN_EINVAL;
        kept += group_of[c] >= 0;
    }
    if (!kept) return MBN_EINVAL;
    if (groups > MBN_CONFUSION_MAX_CLASSES) return MBN_EUNSUPPORTED;
    int n = 0;
    for (int g = 0; g < groups; g++) {                          /* groups ascending, classes ascending inside a group */
        const int first = n;
        for (int c = 0; c < classes; c++)
            if (group_of[c] == g) slot_class[n++] = c;
        if (n == first) continue;                               /* an empty group has no slots and is never a label */
        while (n % 4) slot_class[n++] = -1;
        for (int q = first / 4; q < n / 4; q++) quad_group[q] = q == n / 4 - 1 ? g : -1;
    }
    *slots = n;
    return MBN_OK;
}
