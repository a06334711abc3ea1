"""Writes tests/golden/kernel_cl_vectors.npz and kernel_cl_shapes.txt: the launches of tests/kernel_cl_cases.py run through
the reference's own kernel.cl compiled for the CPU (oracle/_ref/libkernel_cl.so: `make -C oracle` on a machine that has
the reference). The files hold data only — inputs, filters, arguments, NDRange and the bytes the compiled reference wrote —
so the GPU tests need neither the reference nor oracle/_ref/.

    python tests/golden/make_kernel_cl_fixtures.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import kernel_cl  # noqa: E402
import kernel_cl_cases as kc  # noqa: E402


def main():
    if not kernel_cl.available():
        raise SystemExit("oracle/_ref/libkernel_cl.so is missing: run `make -C oracle` where the reference is present")
    cases, by_name = kc.specs(), {}
    for c in cases:
        if c["prev"]:
            c["x"] = by_name[c["prev"]]["want"]
        c["want"] = kc.run_reference(kernel_cl, c)
        by_name[c["name"]] = c
        w = c["want"]
        print("%-30s quirks 0x%X  %6d bytes out, %5.1f %% non-zero, %3d distinct" % (
            c["name"], kc.quirks_of(c), w.size, 100.0 * (w != 0).mean(), len(set(w.tolist()))))
    kc.save(cases)
    with open(kc.SHAPES, "w") as fp:
        fp.write("# launches of kernel_cl_vectors.npz for oracle/ref_selftest.c (written by make_kernel_cl_fixtures.py):\n"
                 "# kernel per_channel g0 g1 rows cols filtersize stride op_size in_bytes\n")
        for c in cases:
            fp.write(kc.shape_line(c) + "\n")
    print("%s: %d cases, %d bytes" % (os.path.basename(kc.VECTORS), len(cases), os.path.getsize(kc.VECTORS)))


if __name__ == "__main__":
    main()
