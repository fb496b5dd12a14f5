"""The compiler's kernel resource report in the form kept under profiles/*/resource_*.txt.

    hipcc <the Makefile's flags> --cuda-device-only -Rpass-analysis=kernel-resource-usage \
        -c csrc/FILE.hip -o /dev/null 2> remarks.txt
    python scripts/resource_report.py remarks.txt [name-filter] > resource.txt

Drops the `file:line:col: remark:` prefix, sorts the records by mangled kernel
name, and keeps only kernels whose name contains `name-filter` when given.
"""
import re
import sys


def main():
    text = open(sys.argv[1]).read()
    want = sys.argv[2] if len(sys.argv) > 2 else ""
    recs, cur = {}, None
    for line in text.splitlines():
        m = re.match(r".*?: remark: (.*)$", line)
        if not m:
            continue
        body = re.sub(r"\s*\[-Rpass-analysis=[^\]]*\]$", "", m.group(1))
        if body.startswith("Function Name:"):
            cur = body.split(":", 1)[1].strip()
            recs[cur] = [body]
        elif cur is not None and body.strip():
            recs[cur].append("    " + body.strip())
    for name in sorted(recs):
        if want in name:
            print("\n".join(recs[name]))


if __name__ == "__main__":
    main()
