#!/usr/bin/env python3
"""Every `File.scala:N` / `File.scala:N-M` citation in the repo points inside the cited file.

A developer check, run by hand where a checkout of the reference (dzufferey/round) exists:

    python scripts/check_citations.py PATH/TO/REFERENCE

The reference is read as text only (line counts). A citation may name a path suffix
(`example/Otr.scala:13`, `psync/Round.scala:57`) or a bare file name; with several
reference files of that name the citation must fit at least one of them. Not part of the
test suite: the suite reads nothing outside the repository.
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CITE = re.compile(r"([A-Za-z0-9_./-]*?)([A-Za-z0-9_]+\.scala):(\d+)(?:-(\d+))?")
SCAN_EXT = (".py", ".hip", ".hpp", ".cpp", ".h", ".c", ".md", ".scala", ".sh")
SKIP_DIRS = {".git", "build", "__pycache__", ".pytest_cache", "profiles"}
# files written by others (survey / judge / advisor reviews) are not the build's citations
SKIP_FILES = {"SURVEY.md", "VERDICT.md", "ADVICE.md", "PAPERS.md", "SNIPPETS.md", "BASELINE.md"}


def ref_files(ref):
    out = {}
    for dp, _, fs in os.walk(ref):
        for f in fs:
            if f.endswith(".scala"):
                p = os.path.join(dp, f)
                with open(p, encoding="utf-8", errors="replace") as fh:
                    out.setdefault(f, []).append((p, sum(1 for _ in fh)))
    return out


def check(ref_root):
    """(citations checked, list of out-of-range or unresolvable ones)."""
    ref = ref_files(ref_root)
    bad = []
    checked = 0
    for dp, dns, fs in os.walk(ROOT):
        dns[:] = [d for d in dns if d not in SKIP_DIRS and not d.startswith(".")]
        for f in fs:
            if not f.endswith(SCAN_EXT) or f in SKIP_FILES:
                continue
            path = os.path.join(dp, f)
            with open(path, encoding="utf-8", errors="replace") as fh:
                for ln, line in enumerate(fh, 1):
                    for m in CITE.finditer(line):
                        prefix, base, a, b = m.group(1), m.group(2), int(m.group(3)), m.group(4)
                        hi = int(b) if b else a
                        cands = ref.get(base, [])
                        if prefix:
                            suffix = prefix.rstrip("/").split("/")[-1]
                            narrowed = [c for c in cands if f"/{suffix}/" in c[0]]
                            cands = narrowed or cands
                        if not cands:
                            bad.append(f"{os.path.relpath(path, ROOT)}:{ln}: {m.group(0)} (no such reference file)")
                            continue
                        checked += 1
                        if not any(1 <= a <= hi <= n for _, n in cands):
                            sizes = ", ".join(f"{os.path.relpath(p, ref_root)} has {n}" for p, n in cands)
                            bad.append(f"{os.path.relpath(path, ROOT)}:{ln}: {m.group(0)} ({sizes})")
    return checked, bad


def main(argv):
    if len(argv) != 1 or not os.path.isdir(argv[0]):
        raise SystemExit(__doc__)
    checked, bad = check(os.path.abspath(argv[0]))
    print(f"{checked} citations checked, {len(bad)} out of range")
    if bad:
        print("\n".join(bad))
    return 1 if bad or checked <= 100 else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
