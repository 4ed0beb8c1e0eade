"""Python mirror of the closed forms of a group's matrix element (csrc/naqs_closed.hpp): the class of a group from its masks
alone, the D and S tables, and both evaluations.  Plain Python integers and floats: every sum is a sequence of IEEE double
adds in ascending term order, as in the C++ builder and in the kernels' term loop."""
import numpy as np

SEG_BITS = 6
SEG_SIZE = 1 << SEG_BITS
CLASS_L, CLASS_D, CLASS_S = 0, 1, 2


def popc(v):
    return bin(int(v)).count("1")


def n_segments(n_qubits):
    return (n_qubits + SEG_BITS - 1) // SEG_BITS


def groups(xy, yz, coeff):
    """[(xy, [yz_t], [c_t])] in ascending xy, terms in ascending input position (naqs_terms_group's order)."""
    xy = np.asarray(xy, np.uint64)
    order = np.argsort(xy, kind="stable")
    out = []
    for k in order:
        if not out or out[-1][0] != int(xy[k]):
            out.append((int(xy[k]), [], []))
        out[-1][1].append(int(yz[k]))
        out[-1][2].append(float(coeff[k]))
    return out


def classify(xy, yzs):
    """(class, R, flipped positions).  R: the first term minimising the largest popc((yz_t ^ R) & ~xy)."""
    nflip = popc(xy)
    if nflip not in (2, 4) or not yzs:
        return CLASS_L, 0, []
    best, ref = None, 0
    for r, yr in enumerate(yzs):
        worst = max(popc((y ^ yr) & ~xy) for y in yzs)
        if best is None or worst < best:
            best, ref = worst, r
    if not ((nflip == 4 and best == 0) or (nflip == 2 and best <= 1)):
        return CLASS_L, 0, []
    return (CLASS_D if nflip == 4 else CLASS_S), yzs[ref], [q for q in range(64) if (xy >> q) & 1]


def deposit(pos, pattern):
    return sum(1 << q for i, q in enumerate(pos) if (pattern >> i) & 1)


def pattern_of(key, pos):
    return sum(((int(key) >> q) & 1) << i for i, q in enumerate(pos))


def build_d(R, pos, yzs, cs):
    T = []
    for p in range(16):
        dep, acc = deposit(pos, p), 0.0
        for y, c in zip(yzs, cs):
            acc += -c if popc(dep & (y ^ R)) & 1 else c
        T.append(acc)
    return T


def build_s(xy, R, pos, yzs, cs, nseg):
    """B[segment][pattern][slice]"""
    B = np.zeros((nseg, 4, SEG_SIZE))
    for p in range(4):
        dep = deposit(pos, p)
        for s in range(nseg):
            for v in range(SEG_SIZE):
                acc = 0.0
                for y, c in zip(yzs, cs):
                    d = y ^ R
                    sp = d & ~xy
                    r = (sp & -sp).bit_length() - 1 if sp else 0
                    if r // SEG_BITS != s:
                        continue
                    par = popc(dep & d) + (((v >> (r - s * SEG_BITS)) & 1) if sp else 0)
                    acc += -c if par & 1 else c
                B[s, p, v] = acc
    return B


def loop_element(key, yzs, cs):
    """The term loop: sum_t c_t (-1)^popc(key & yz_t), ascending t from 0.0."""
    acc = 0.0
    for y, c in zip(yzs, cs):
        acc += -c if popc(int(key) & y) & 1 else c
    return acc


def eval_d(key, R, pos, T):
    h = T[pattern_of(key, pos)]
    return -h if popc(int(key) & R) & 1 else h


def eval_s(key, R, pos, B):
    p = pattern_of(key, pos)
    h = float(B[0, p, int(key) & (SEG_SIZE - 1)])
    for s in range(1, B.shape[0]):
        h += float(B[s, p, (int(key) >> (s * SEG_BITS)) & (SEG_SIZE - 1)])
    return -h if popc(int(key) & R) & 1 else h


def handle_counts(xy, yz, coeff, n_qubits, chunk_terms, max_bytes=4096 * 1024, heavy_terms=8, max_units=1 << 12):
    """(D, S, L, table bytes) as a handle reports them (naqs_ham_closed_counts): the classes walked in the handle's group
    order ([more than heavy_terms terms][the others], each in ascending mask), a D group only if it fits one chunk, a group
    only while the tables stay within max_bytes, an S table only if it begins below the word's unit field."""
    gs = [g for g in groups(xy, yz, coeff)]
    has_diag = 1 if gs and gs[0][0] == 0 else 0
    nd = [g for g in gs if g[0]]
    order = [g for g in nd if len(g[1]) > heavy_terms] + [g for g in nd if len(g[1]) <= heavy_terms]
    nseg = n_segments(n_qubits)
    s_units = 4 * nseg
    classes, used = [], 0
    for gxy, yzs, _ in order:
        cls = classify(gxy, yzs)[0]
        if cls == CLASS_D and len(yzs) > chunk_terms:
            cls = CLASS_L
        add = (16 + (s_units * SEG_SIZE if cls == CLASS_S else 0)) * 8
        if cls != CLASS_L and used + add > max_bytes:
            cls = CLASS_L
        if cls != CLASS_L:
            used += add
        classes.append(cls)
    n_closed = sum(c != CLASS_L for c in classes)
    units = ((has_diag + n_closed) * 16 + SEG_SIZE - 1) // SEG_SIZE
    for i, c in enumerate(classes):
        if c == CLASS_S:
            if units + s_units > max_units:
                classes[i] = CLASS_L
            else:
                units += s_units
    n = [classes.count(CLASS_L), classes.count(CLASS_D), classes.count(CLASS_S)]
    return n[CLASS_D], n[CLASS_S], n[CLASS_L], (units * SEG_SIZE * 8 if n[CLASS_D] + n[CLASS_S] else 0)
