#!/usr/bin/env python3
"""The multiset of message literals the host units pass to fail( and hipfail( (check 3).

    python scripts/fail_literals.py [csrc-dir] > after.txt     # this tree
    python scripts/fail_literals.py <parent>/orleans_amd/csrc > before.txt
    diff before.txt after.txt

Covers orl_api.cpp, the api_*.cpp units and orl_ctx.h.  A call of need_device( or check_batch( counts as one use of that
helper's literal (the helpers expanded), the definition itself as none, so the two outputs are equal exactly when no
message was gained, lost or changed.  Prints "count<TAB>literal", sorted.

A one-off, tied to the shape of orl_ctx.h as it stands: each helper is "inline int NAME(...) { ... fail(c, CODE, "...") ... }"
closed by a brace in column 0, and a helper's name followed by "(" anywhere outside a comment is a call of it."""
import collections
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
csrc = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "orleans_amd", "csrc")
files = sorted(glob.glob(os.path.join(csrc, "api_*.cpp"))) + [os.path.join(csrc, f) for f in ("orl_ctx.h", "orl_api.cpp")]

STRING = r'"(?:[^"\\\n]|\\.)*"'
# fail(c, CODE, "..." ["..."]*   and   hipfail(c, e, "...")   — adjacent literals are one message
CALL = re.compile(r'\b(hip)?fail\(\s*\(?\w+\)?\s*,\s*[^,;"]+,\s*((?:%s\s*)+)' % STRING)
HELPERS = {"need_device": None, "check_batch": None}

counts = collections.Counter()
calls = collections.Counter()
for path in files:
    if not os.path.exists(path):
        continue
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(path).read(), flags=re.S)
    for name in HELPERS:  # the helper's own literal: found in its definition, counted per call
        m = re.search(r"inline int %s\([^)]*\)\s*\{(.*?)\n\}" % name, text, flags=re.S)
        if m:
            lit = CALL.search(m.group(1))
            assert lit, "%s in %s holds no fail( literal: this script no longer fits the header" % (name, path)
            HELPERS[name] = "".join(s[1:-1] for s in re.findall(STRING, lit.group(2)))
            text = text.replace(m.group(0), "")
        calls[name] += len(re.findall(r"\b%s\(" % name, text))
    for m in CALL.finditer(text):
        counts["".join(s[1:-1] for s in re.findall(STRING, m.group(2)))] += 1
for name, lit in HELPERS.items():
    if lit is not None:
        counts[lit] += calls[name]
for lit, n in sorted(counts.items()):
    print("%d\t%s" % (n, lit))
print("# %d calls, %d distinct literals" % (sum(counts.values()), len(counts)), file=sys.stderr)
