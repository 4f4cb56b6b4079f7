"""A filter program (include/icd_search.h) interpreted in plain numpy over whole columns: what the program
SAYS, not how the kernel walks it. cols: int [ncols, n]; text(terms, m) -> bool[n] evaluates a TEXT leaf (tests pass
text_match_oracle.match_rows over the sparse rows). Returns the sorted int64 row ids of the one set the program leaves."""
import numpy as np


def run(prog, cols, text=None):
    cols = np.asarray(cols)
    n, stack, pc = cols.shape[1], [], 0
    prog = [int(w) for w in np.asarray(prog).reshape(-1)]
    i32 = lambda w: w - (1 << 32) if w >= 1 << 31 else w   # noqa: E731
    while pc < len(prog):
        w = prog[pc]
        op, count, m = w & 0xFF, (w >> 8) & 0xFF, w >> 16
        if op == 1:
            c = cols[prog[pc + 1]].astype(np.int64)
            stack.append((c >= i32(prog[pc + 2])) & (c < i32(prog[pc + 3])))
            pc += 4
        elif op == 2:
            stack.append(np.isin(cols[prog[pc + 1]].astype(np.int64), [i32(x) for x in prog[pc + 2:pc + 2 + count]]))
            pc += 2 + count
        elif op == 3:
            stack.append(np.asarray(text(prog[pc + 1:pc + 1 + count], m), bool) if m <= count else np.zeros(n, bool))
            pc += 1 + count
        elif op in (4, 5):
            b, a = stack.pop(), stack.pop()
            stack.append(a & b if op == 4 else a | b)
            pc += 1
        else:
            assert op == 6, op
            stack.append(~stack.pop())
            pc += 1
    assert len(stack) == 1
    return np.flatnonzero(stack[0]).astype(np.int64)
