"""Per-kernel medians of the input path from a kernel trace of tools/input_time.py (profiles/input_kernels.txt).

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/input_time.py --kernels-only
    python tools/input_kernels.py DIR/*/*_results.db > profiles/input_kernels.txt

--kernels-only runs the 513^2 arms first and the 200^2 arms after them, every arm the same number of times, one after the
other in each round.  So a kernel's dispatches in time order split in halves by size, and the dispatches of a kernel that
several arms launch (k_augment_ex: rotation only, jitter without contrast, jitter with contrast, all on; k_augment_gray_sum:
the last two) cycle through those arms.  Warm-up calls are counted like the timed ones."""
import collections
import sqlite3
import statistics
import sys

from input_time import EXT_ARMS

ARMS = {"k_augment_ex": [a for a, _ in EXT_ARMS],
        "k_augment_gray_sum": [a for a, kw in EXT_ARMS if kw.get("jitter", (0, 0))[1]]}
ORDER = ("k_label_prepare", "k_count_finalize<1>", "k_augment", "k_aug_tables", "k_aug_rotate", "k_augment_ex",
         "k_augment_gray_sum", "k_augment_gray_mean", "k_gather_normalize")


def main(db):
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    runs = collections.defaultdict(list)
    for name, start, end in rows:
        if "iswm::" in name:
            runs[name.split("(")[0].replace("void ", "").replace("iswm::", "")].append((end - start) / 1e3)
    print("rocprofv3 --kernel-trace --stats -- python tools/input_time.py --kernels-only   (one MI355X; batch 16; 4 warm-up + 5 timed")
    print("calls of every arm per size; a run of its own), summarised by tools/input_kernels.py")
    print("%-22s %-40s %5s %10s %10s %10s" % ("kernel", "case", "calls", "median us", "min us", "max us"))
    for half, size in enumerate(("513^2 crop 513", "200^2 crop 200")):
        for k in ORDER:
            v = runs.get(k, [])
            v = v[:len(v) // 2] if half == 0 else v[len(v) // 2:]
            arms = ARMS.get(k, [None])
            for i, arm in enumerate(arms):
                part = v[i::len(arms)]
                if part:
                    print("%-22s %-40s %5d %10.1f %10.1f %10.1f" % (k, size + (", " + arm if arm else ""), len(part),
                                                                   statistics.median(part), min(part), max(part)))


if __name__ == "__main__":
    main(sys.argv[1])
