"""Shared by the tests/test_gpu_fp16_*.py files and scripts/make_golden_fp16.py (not a test module): the one writer of
tests/golden/REPORT_fp16.txt, a header and one section per source."""
import os
import re

REPORT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "REPORT_fp16.txt")


def report_section(mark, lines):
    """Replace the section `mark` of the report (sections: a '== ' line up to the next one) by `lines`, keeping the others."""
    try:
        text = open(REPORT).read() if os.path.exists(REPORT) else ""
        head, *secs = re.split(r"(?m)^(?=== )", text)
        secs = {s.split("\n", 1)[0] + "\n": s for s in secs}
        secs[mark] = mark + "".join(lines)
        head = head or ("One-piece fp16 arithmetic (\"fp16\": x^ = fp16_rne(x * 2^xs), w^ = fp16_rne(w * 2^s), one product per K step, fp32\n"
                        "accumulation) on MI355X.  Written by the tests named in each section.\n")
        with open(REPORT, "w") as f:
            f.write(head + "".join(secs[k] for k in sorted(secs)))
    except OSError:
        pass  # a read-only checkout: the figures were printed
