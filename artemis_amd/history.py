"""Reader of the history files the host driver writes (<problem_id>.outN.hst, include/artemis_driver.h "deck-driven
outputs"): a section starts with the line "#  History data", followed by the label line "# [1]=time [2]=dt ..." and
one whitespace-separated row per output.  A run that appends to an existing file starts a new section."""
import numpy as np

HEADER = "#  History data"


def read_history(path):
    """{label: ndarray} of the LAST section of a history file, one entry per column in file order (integers such as
    `cycle` and `nbtotal` come back as floats, like every other column)."""
    with open(path) as f:
        lines = f.read().split("\n")
    starts = [n for n, ln in enumerate(lines) if ln.strip() == HEADER]
    if not starts:
        raise ValueError("%s is not a history file: no '%s' line" % (path, HEADER))
    s = starts[-1]
    if s + 1 >= len(lines) or not lines[s + 1].startswith("#"):
        raise ValueError("%s: the last section has no label line" % path)
    labels = []
    for n, tok in enumerate(lines[s + 1][1:].split()):
        head, eq, name = tok.partition("=")
        if head != "[%d]" % (n + 1) or not eq or not name:
            raise ValueError("%s: bad label %r" % (path, tok))
        labels.append(name)
    rows = []
    for ln in lines[s + 2:]:
        if not ln.strip() or ln.lstrip().startswith("#"):
            continue
        vals = ln.split()
        if len(vals) != len(labels):
            raise ValueError("%s: a row has %d columns, the label line %d" % (path, len(vals), len(labels)))
        rows.append([float(v) for v in vals])
    data = np.array(rows, dtype=np.float64).reshape(len(rows), len(labels))
    return {name: data[:, n].copy() for n, name in enumerate(labels)}
