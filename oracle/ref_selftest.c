/*
 * ref_selftest.c — `make -C oracle ref-selftest`: the reference's kernel.cl and kernel_cl_driver.c linked into
 * a plain executable under AddressSanitizer and UndefinedBehaviorSanitizer. TEST INFRASTRUCTURE ONLY.
 *
 * Reads the launches that tests/golden/kernel_cl_vectors.npz records (tests/golden/kernel_cl_shapes.txt, one per
 * line, written by the same generator) and makes each of them in heap buffers of exactly the size the guard
 * arithmetic of kernel_cl_driver.c gives (what oracle/kernel_cl.py allocates): inputs grown by zeros to the
 * largest index read, the filter at the taps consumed, the output at the call's own size. A read or write
 * outside those sizes is a sanitizer report and a non-zero exit; so is a launch whose bytes depend on the
 * work-item order. Exit 0 = the guard sizing keeps every recorded launch in bounds.
 *
 * line:  kernel per_channel g0 g1 rows cols filtersize stride op_size in_bytes
 *        in_bytes = bytes of the input buffer (of each of the three for convolute) before the guard
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void ref_convolute(int, int, int, unsigned char *, unsigned char *, unsigned char *, unsigned char *, int *, int, int, int,
                   int, int);
void ref_depthwise(int, int, int, unsigned char *, unsigned char *, int *, int, int, int, int, int);
void ref_pointwise(int, int, int, unsigned char *, unsigned char *, int *, int, int, int, int);
void ref_pool(int, int, int, unsigned char *, unsigned char *, int, int, int, int);
long ref_max_in_window(int, int, int, int);
long ref_taps(int);
long ref_max_in_pointwise(int, int, int, int, int);
long ref_max_in_pool(int, int, int, int);
long ref_max_out(int, int, long, int);

static unsigned rnd_state = 12345u;
static unsigned rnd(void) { return rnd_state = rnd_state * 1664525u + 1013904223u; }

static unsigned char *input(long data, long total)
{
    unsigned char *p = calloc((size_t)total, 1);
    if (!p) exit(2);
    for (long i = 0; i < data; i++) p[i] = (unsigned char)(rnd() >> 24);
    return p;
}

static long max2(long a, long b) { return a > b ? a : b; }

static int run_line(const char *k, int pc, int g0, int g1, int rows, int cols, int fs, int stride, int op, long in_bytes)
{
    const int is_conv = !strcmp(k, "convolute"), is_dw = !strcmp(k, "depthwise"), is_pw = !strcmp(k, "pointwise"),
              is_pool = !strcmp(k, "pool");
    if (!(is_conv || is_dw || is_pw || is_pool)) return 1;
    const long shift = is_conv ? (long)(rows / 2) * (cols / 2) : is_pool ? 1 : (long)rows * cols;
    const long taps = is_conv ? 3 * ref_taps(fs) : is_dw ? ref_taps(fs) : is_pw ? fs : 0;
    const long out_size = shift * op;
    const int calls = pc ? op : 1, n = pc ? 1 : op;
    const long in_plane = is_dw ? in_bytes / op : (long)rows * cols;
    const long in_step = pc && (is_dw || is_pool) ? in_plane : 0;    /* pointwise: the input stays at plane 0 */
    const long reach = is_pw ? ref_max_in_pointwise(g0, g1, rows, cols, fs) : is_pool ? ref_max_in_pool(rows, cols, fs, n)
                                                                            : ref_max_in_window(g0, g1, fs, stride);
    const long out_reach = ref_max_out(g0, g1, shift, n);
    if (reach < 0 || out_reach < 0 || taps < 0) return 1;
    if (shift * (calls - 1) + out_reach + 1 > out_size) return 1;     /* the launch would write past its output */
    const long in_total = max2(in_bytes, in_step * (calls - 1) + reach + 1);
    unsigned char *in[3] = { input(in_bytes, in_total), is_conv ? input(in_bytes, in_total) : NULL,
                             is_conv ? input(in_bytes, in_total) : NULL };
    int *filt = malloc((size_t)(taps * op + 1) * sizeof(int));
    unsigned char *out[2] = { malloc((size_t)out_size), malloc((size_t)out_size) };
    if (!filt || !out[0] || !out[1]) exit(2);
    for (long i = 0; i < taps * op; i++) filt[i] = (int)(rnd() >> 8) % 7 - 3;
    for (int order = 0; order < 2; order++) {
        memset(out[order], 0x5a, (size_t)out_size);
        for (int c = 0; c < calls; c++) {
            unsigned char *o = out[order] + shift * c;
            int *f = filt + taps * c;
            if (is_conv) ref_convolute(g0, g1, order, o, in[0], in[1], in[2], f, rows, cols, fs, stride, n);
            else if (is_dw) ref_depthwise(g0, g1, order, o, in[0] + in_step * c, f, rows, cols, fs, stride, n);
            else if (is_pw) ref_pointwise(g0, g1, order, o, in[0], f, rows, cols, fs, n);
            else ref_pool(g0, g1, order, o, in[0] + in_step * c, rows, cols, fs, n);
        }
    }
    const int differ = memcmp(out[0], out[1], (size_t)out_size) != 0;
    free(in[0]); free(in[1]); free(in[2]); free(filt); free(out[0]); free(out[1]);
    return differ;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s kernel_cl_shapes.txt\n", argv[0]); return 2; }
    FILE *fp = fopen(argv[1], "r");
    if (!fp) { perror(argv[1]); return 2; }
    char line[256], k[32];
    int launches = 0;
    while (fgets(line, sizeof line, fp)) {
        int pc, g0, g1, rows, cols, fs, stride, op;
        long in_bytes;
        if (line[0] == '#' || line[0] == '\n') continue;
        if (sscanf(line, "%31s %d %d %d %d %d %d %d %d %ld", k, &pc, &g0, &g1, &rows, &cols, &fs, &stride, &op, &in_bytes) != 10) {
            fprintf(stderr, "ref_selftest: cannot read: %s", line);
            return 2;
        }
        if (run_line(k, pc, g0, g1, rows, cols, fs, stride, op, in_bytes)) {
            fprintf(stderr, "ref_selftest: out of the guard arithmetic, or order-dependent: %s", line);
            return 1;
        }
        launches++;
    }
    fclose(fp);
    if (!launches) { fprintf(stderr, "ref_selftest: no launches in %s\n", argv[1]); return 2; }
    printf("ref_selftest: %d launches in bounds and order-independent\n", launches);
    return 0;
}
