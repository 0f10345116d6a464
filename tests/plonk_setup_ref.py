"""Reference restatement of plonk.Setup's scalar half, line by line from
backend/plonk/bls12-381/setup.go (the bn254 file is the same text): initDomains
(:275-290), BuildTrace (:173-225), buildPermutation (:304-358),
computePermutationPolynomials / getSupportPermutation (:363-407), and the
definition of the Lagrange SRS as a double sum.  Plain Python ints, written
from the Go text and not from csrc/plonk_setup.hip.

A constraint is (xa, xb, xc, qL, qR, qO, qM, qC) as in oracle/scs_solver.py;
commitments: [(committed constraint indices, commitment constraint index)].
"""


def next_pow2(x):
    n = 1
    while n < x:
        n <<= 1
    return n


def init_domains(n_constraints, nb_public):
    """(n, big): setup.go:275-290.  fft.NewDomain rounds up to a power of two."""
    size_system = n_constraints + nb_public
    n = next_pow2(size_system)
    if size_system < 6:
        big = next_pow2(8 * size_system)
    else:
        big = next_pow2(4 * size_system)
    return n, big


def build_trace(mod, cons, nb_public, commitments=()):
    """ql, qr, qm, qo, qk, [qcp_j]: Lagrange regular ints (setup.go:175-225)."""
    size_system = len(cons) + nb_public
    size = next_pow2(size_system)
    ql, qr, qm, qo, qk = ([0] * size for _ in range(5))
    for i in range(nb_public):
        ql[i] = mod - 1
    offset = nb_public
    for j, (_xa, _xb, _xc, qL, qR, qO, qM, qC) in enumerate(cons):
        ql[offset + j] = qL % mod
        qr[offset + j] = qR % mod
        qm[offset + j] = qM % mod
        qo[offset + j] = qO % mod
        qk[offset + j] = qC % mod
    qcp = []
    for committed, _idx in commitments:
        q = [0] * size
        for k in committed:
            q[offset + k] = 1
        qcp.append(q)
    return ql, qr, qm, qo, qk, qcp


def build_lro(cons, nb_public, size):
    """position -> variable id (setup.go:317-332); the slots nobody writes stay 0"""
    lro = [0] * (3 * size)
    for i in range(nb_public):
        lro[i] = i
    offset = nb_public
    for j, k in enumerate(cons):
        lro[offset + j] = k[0]
        lro[size + offset + j] = k[1]
        lro[2 * size + offset + j] = k[2]
    return lro


def build_permutation(cons, nb_public, nb_variables):
    """pt.S (setup.go:304-358)"""
    size = next_pow2(len(cons) + nb_public)
    lro = build_lro(cons, nb_public, size)
    permutation = [-1] * (3 * size)
    cycle = [-1] * nb_variables
    for i in range(len(lro)):
        if cycle[lro[i]] != -1:
            permutation[i] = cycle[lro[i]]
        cycle[lro[i]] = i
    for i in range(3 * size):
        if permutation[i] == -1:
            permutation[i] = cycle[lro[i]]
    return permutation


def support_permutation(mod, n, omega, u):
    """<g> || u<g> || u^2<g> (setup.go:392-407)"""
    res = [0] * (3 * n)
    res[0], res[n], res[2 * n] = 1, u % mod, u * u % mod
    for i in range(1, n):
        res[i] = res[i - 1] * omega % mod
        res[n + i] = res[n + i - 1] * omega % mod
        res[2 * n + i] = res[2 * n + i - 1] * omega % mod
    return res


def permutation_polynomials(mod, perm, n, omega, u):
    """S1, S2, S3 in Lagrange regular form (setup.go:363-388)"""
    ident = support_permutation(mod, n, omega, u)
    return ([ident[perm[i]] for i in range(n)], [ident[perm[n + i]] for i in range(n)],
            [ident[perm[2 * n + i]] for i in range(n)])


def to_lagrange_ref(cv, points, omega):
    """out[i] = (1/n) sum_j omega^(-ij) points[j] with the oracle's big-int point
    arithmetic (cv: plonk_prover_oracle.Curve); the defining double sum, n <= 16."""
    n = len(points)
    assert n <= 16
    R = cv.R
    winv, ninv = pow(omega, -1, R), pow(n, -1, R)
    out = []
    for i in range(n):
        acc = cv.INF
        for j in range(n):
            acc = cv.add(acc, cv.mul(points[j], pow(winv, i * j, R) * ninv % R))
        out.append(acc)
    return out


def lagrange_at(mod, n, omega, tau):
    """[L_i(tau)] for i < n by the closed form w^i (tau^n - 1) / (n (tau - w^i))"""
    c = (pow(tau, n, mod) - 1) * pow(n, -1, mod) % mod
    out, wi = [], 1
    for _ in range(n):
        out.append(wi * c % mod * pow((tau - wi) % mod, -1, mod) % mod)
        wi = wi * omega % mod
    return out
