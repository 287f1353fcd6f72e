"""The R1CS front end's mapping ("layout 1": include/sonic_hip.h, "R1CS front end") as a Python-integer model: the reference for every
byte that sonic_amd/csrc/r1cs.hpp lays out and sonic_amd/csrc/r1cs.hip computes.

A matrix is a list of m rows, a row a list of (column, value) pairs with strictly increasing columns (explicit zeros stay entries).
Column 0 is the constant one, columns 1..n_pub the public inputs.  n = m + N // 2 gates, Q = 3m + n_pub linear constraints; the compiled
system is a list of 3Q rows (wL rows, wR rows, wO rows) of (gate, weight) pairs plus the constants cs.
"""
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def shape(m, N, n_pub):
    """(n, Q, g)"""
    g = N // 2
    return m + g, 3 * m + n_pub, g


def home(m, j):
    """variable j >= 1 -> (0: wL / aL, 1: wR / aR; gate)"""
    return (j - 1) % 2, m + (j - 1) // 2


def compile_r1cs(m, N, n_pub, A, B, C):
    """-> (rows, cs_fixed): 3Q rows of (gate, weight) pairs, Q constants with the public slots zero"""
    n, Q, _ = shape(m, N, n_pub)
    rows = [[] for _ in range(3 * Q)]
    cs = [0] * Q
    for k, M in enumerate((A, B, C)):
        for i in range(m):
            q = k * m + i
            rows[k * Q + q].append((i, 1))
            for j, v in M[i]:
                if j == 0:
                    cs[q] = v % R
                    continue
                w, gate = home(m, j)
                rows[w * Q + q].append((gate, (-v) % R))
    for k in range(1, n_pub + 1):
        w, gate = home(m, k)
        rows[w * Q + 3 * m + k - 1].append((gate, 1))
    return rows, cs


def csr_of(rows):
    """-> (row_ptr, col, val) of a list of rows"""
    row_ptr, col, val = [0], [], []
    for row in rows:
        col += [c for c, _ in row]
        val += [v for _, v in row]
        row_ptr.append(len(col))
    return row_ptr, col, val


def nnz_formula(m, n_pub, A, B, C):
    total = sum(len(r) for M in (A, B, C) for r in M)
    col0 = sum(1 for M in (A, B, C) for r in M for j, _ in r if j == 0)
    return total - col0 + 3 * m + n_pub


def dot(row, z):
    return sum(v * z[j] for j, v in row) % R


def assign(m, N, n_pub, A, B, C, z):
    """one witness -> (aL, aR, aO, cs, (broken constraint gates, the first or -1))"""
    n, Q, g = shape(m, N, n_pub)
    z = [v % R for v in z]
    aL = [dot(A[i], z) for i in range(m)]
    aR = [dot(B[i], z) for i in range(m)]
    aO = [dot(C[i], z) for i in range(m)]
    broken = [i for i in range(m) if aL[i] * aR[i] % R != aO[i]]
    for t in range(g):
        l, r = z[2 * t + 1], (z[2 * t + 2] if 2 * t + 2 < N else 0)
        aL.append(l)
        aR.append(r)
        aO.append(l * r % R)
    _, cs = compile_r1cs(m, N, n_pub, A, B, C)
    for k in range(1, n_pub + 1):
        cs[3 * m + k - 1] = z[k]
    return aL, aR, aO, cs, (len(broken), broken[0] if broken else -1)


def sonic_holds(Q, rows, cs, aL, aR, aO):
    """every linear constraint and every multiplication gate of the compiled system"""
    for q in range(Q):
        s = sum(w * aL[c] for c, w in rows[q]) + sum(w * aR[c] for c, w in rows[Q + q]) + sum(w * aO[c] for c, w in rows[2 * Q + q])
        if (s - cs[q]) % R:
            return False
    return all((aL[i] * aR[i] - aO[i]) % R == 0 for i in range(len(aL)))


def r1cs_holds(A, B, C, z):
    return all((dot(A[i], z) * dot(B[i], z) - dot(C[i], z)) % R == 0 for i in range(len(A)))


def random_row(rng, N, count, coeffs=None):
    cols = sorted(rng.sample(range(N), min(count, N)))
    pick = coeffs or (lambda: rng.choice([1, R - 1, rng.randrange(R)]))
    return [(j, pick()) for j in cols]


def random_r1cs(rng, m, N, n_pub, lengths=None, z=None, coeffs=None):
    """a satisfiable system and its witness: A and B rows are random, a C row is random but for one coefficient (on a column where z is
    non-zero; column 0 if need be), which is solved for.  lengths: per row (len A, len B, len C), default 0..4 each"""
    z = list(z) if z is not None else [1] + [rng.randrange(R) for _ in range(N - 1)]
    A, B, C = [], [], []
    for i in range(m):
        la, lb, lc = lengths[i] if lengths else (rng.randrange(5), rng.randrange(5), rng.randrange(5))
        a, b, c = random_row(rng, N, la, coeffs), random_row(rng, N, lb, coeffs), random_row(rng, N, lc, coeffs)
        want = dot(a, z) * dot(b, z) % R
        if dot(c, z) != want:
            nz = [k for k, (j, _) in enumerate(c) if z[j] % R]
            if not nz:
                c = sorted(c + [(0, 0)]) if all(j != 0 for j, _ in c) else c
                nz = [k for k, (j, _) in enumerate(c) if z[j] % R]
            k = nz[rng.randrange(len(nz))]
            j = c[k][0]
            rest = (dot(c, z) - c[k][1] * z[j]) % R
            c[k] = (j, (want - rest) * pow(z[j], -1, R) % R)
        A.append(a)
        B.append(b)
        C.append(c)
    return A, B, C, z


def matrix_csr(M):
    """a matrix as (row_ptr, col, val) integer lists"""
    return csr_of(M)
