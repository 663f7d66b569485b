"""TEST INFRASTRUCTURE: an exact integer reference for the field, Z_r and curve kernels -- plain Python ints, no numpy
arithmetic, no ctypes, nothing from the reference tree at run time (numpy only packs the records of a batch).

  Fq(q), Zr(r)            the base field and the scalar ring, op numbering of pbc_hip_fq_op_batch / pbc_hip_zr_op_batch
  Ext(q, modulus)         F_q[X] / (X^d + c(d-1) X^(d-1) + ... + c0): F_q^2 of type f, F_q^3 of type d, F_q^5 of type g;
                          inversion by the extended Euclid algorithm on polynomials
  Curve(field, a, b, r)   the affine group law with the reference's case analysis (curve_mul / curve_double, ecc/curve.c),
                          double-and-add with the scalar taken mod r first, as the reference reads a Z_r record
  family(param text)      G1's and G2's curves and the byte layout of their records; on the twists the curve comes from
                          the parameter text (field_reinit_curve_twist ecc/curve.c:885-901: a nqr^2, b nqr^3 over
                          F_q^d for types d / g; f_param.c:372-383: b' = -(alpha0 + alpha1 sqrt(beta)) b for type f)
  patterns(m, rbits)      the limb patterns oracle/ref_harness.c soak_pattern crafts, as values and as Montgomery residues
  scalars(r, zl)          scalars with structured nibbles for the regular signed 4-bit window recoding
  battery_*(name)         the crafted batches tests/test_crafted_cpu.py and tests/test_gpu_crafted.py share: input records
                          and the bytes this reference expects, computed once per session

tests/test_crafted_cpu.py pins this file to the reference's fixtures before it judges anything."""
import functools
import math

import numpy as np

FQ_OPS = {"mul": 0, "add": 1, "sub": 2, "invert": 3, "neg": 4, "halve": 5, "double": 6}      # pbc_hip_fq_op_batch
ZR_OPS = dict(FQ_OPS, div=7)                                                                  # pbc_hip_zr_op_batch


# ---- fields -------------------------------------------------------------------------------------------------------------
class Fq:
    """integers mod m; elements are ints in [0, m)"""
    d = 1

    def __init__(self, m):
        self.m = m
        self.order = m
        self.zero, self.one = 0, 1 % m

    def embed(self, n):
        return n % self.m

    def coeffs(self, x):
        return [x]

    def from_coeffs(self, c):
        return c[0] % self.m

    def add(self, a, b):
        return (a + b) % self.m

    def sub(self, a, b):
        return (a - b) % self.m

    def neg(self, a):
        return -a % self.m

    def mul(self, a, b):
        return a * b % self.m

    def inv(self, a):
        return pow(a, -1, self.m)

    def halve(self, a):
        a %= self.m
        return (a if a % 2 == 0 else a + self.m) // 2

    def double(self, a):
        return 2 * a % self.m

    def div(self, a, b):
        return a * pow(b, -1, self.m) % self.m

    def pow(self, a, e):
        return pow(a, e, self.m)

    def op(self, op, a, b=None):
        """op of pbc_hip_fq_op_batch on ints of any size (records >= m are reduced on load)"""
        a %= self.m
        b = a if b is None else b % self.m
        return [self.mul, self.add, self.sub, lambda x, y: self.inv(x), lambda x, y: self.neg(x), lambda x, y: self.halve(x),
                lambda x, y: self.double(x), self.div][op](a, b)


class Zr(Fq):
    """the scalar ring (a1: the composite n): the same routines on the modulus r; op 7 = a / b"""


class Ext:
    """F_q[X] / (X^d + modulus[d-1] X^(d-1) + ... + modulus[0]); elements are tuples of d ints, coefficient 0 first"""

    def __init__(self, q, modulus):
        self.q, self.mod, self.d = q, [c % q for c in modulus], len(modulus)
        self.order = q ** self.d
        self.zero = (0,) * self.d
        self.one = (1,) + (0,) * (self.d - 1)
        self._mul = None

    def embed(self, n):
        return (n % self.q,) + (0,) * (self.d - 1)

    def coeffs(self, x):
        return list(x)

    def from_coeffs(self, c):
        return tuple(v % self.q for v in c)

    def add(self, a, b):
        return tuple((x + y) % self.q for x, y in zip(a, b))

    def sub(self, a, b):
        return tuple((x - y) % self.q for x, y in zip(a, b))

    def neg(self, a):
        return tuple(-x % self.q for x in a)

    def double(self, a):
        return tuple(2 * x % self.q for x in a)

    def _reduce(self, p):
        p = list(p)
        for i in range(len(p) - 1, self.d - 1, -1):              # X^i = -sum mod[j] X^(i - d + j)
            c = p[i]
            if c:
                for j in range(self.d):
                    p[i - self.d + j] -= c * self.mod[j]
        return tuple(x % self.q for x in p[:self.d])

    def mul_schoolbook(self, a, b):
        p = [0] * (2 * self.d - 1)
        for i, x in enumerate(a):
            if x:
                for j, y in enumerate(b):
                    p[i + j] += x * y
        return self._reduce(p)

    def mul(self, a, b):
        """the schoolbook product above written out for this d (one expression per coefficient: the loops cost more than
        the integers); X^(d + i) comes reduced from a table"""
        if self._mul is None:
            d = self.d
            red = [self._reduce([0] * (d + i) + [1]) for i in range(d - 1)]
            conv = ["+".join("a[%d]*b[%d]" % (i, k - i) for i in range(d) if 0 <= k - i < d) for k in range(2 * d - 1)]
            body = "".join("    c%d = %s\n" % (k, e) for k, e in enumerate(conv))
            outs = ["(c%d" % j + "".join("+c%d*%d" % (d + i, red[i][j]) for i in range(d - 1)) + ") % q" for j in range(d)]
            ns = {"q": self.q}
            exec("def mul(a, b):\n" + body + "    return (" + ", ".join(outs) + ",)\n", ns)
            self._mul = ns["mul"]
        return self._mul(a, b)

    def inv(self, a):
        """extended Euclid on polynomials over F_q: u a = g mod the modulus, g a non-zero constant"""
        q = self.q

        def trim(p):
            while p and p[-1] == 0:
                p.pop()
            return p
        r0, r1 = self.mod + [1], trim(list(a))
        if not r1:
            raise ZeroDivisionError("0 has no inverse")
        u0, u1 = [], [1]
        while len(r1) > 1:
            inv_lead = pow(r1[-1], -1, q)
            quo = [0] * (len(r0) - len(r1) + 1)
            r0 = list(r0)
            for k in range(len(r0) - len(r1), -1, -1):
                c = r0[k + len(r1) - 1] * inv_lead % q
                quo[k] = c
                if c:
                    for j, y in enumerate(r1):
                        r0[k + j] = (r0[k + j] - c * y) % q
            rem = trim(r0)
            prod = [0] * (len(quo) + len(u1) - 1)                  # u0 - quo u1
            for i, x in enumerate(quo):
                for j, y in enumerate(u1):
                    prod[i + j] += x * y
            nu = [0] * max(len(prod), len(u0))
            for i in range(len(nu)):
                nu[i] = ((u0[i] if i < len(u0) else 0) - (prod[i] if i < len(prod) else 0)) % q
            r0, r1, u0, u1 = r1, rem, u1, trim(nu)
            if not r1:
                raise ZeroDivisionError("not invertible")
        c = pow(r1[0], -1, q)
        u1 = u1 + [0] * (self.d - len(u1))
        return tuple(x * c % q for x in u1[:self.d])

    def pow(self, a, e):
        r = self.one
        for bit in bin(e)[2:]:
            r = self.mul(r, r)
            if bit == "1":
                r = self.mul(r, a)
        return r


def sqrt(F, a):
    """a square root of a in F (Fq or Ext), or None: (order + 1) / 4-th power where order = 3 mod 4, else Tonelli-Shanks
    with the first non-residue of a fixed enumeration"""
    if a == F.zero:
        return a
    Q = F.order
    if Q % 4 == 3:
        y = F.pow(a, (Q + 1) // 4)
        return y if F.mul(y, y) == a else None
    if F.pow(a, (Q - 1) // 2) != F.one:
        return None
    if getattr(F, "_ts", None) is None:                          # (s, t, z^t) with Q - 1 = 2^s t, z the first non-residue found
        s, t = 0, Q - 1
        while t % 2 == 0:
            s, t = s + 1, t // 2
        for c in range(2, 1000):                                 # c (+ X on an extension)
            z = F.embed(c) if F.d == 1 else F.from_coeffs([c, 1] + [0] * (F.d - 2))
            if F.pow(z, (Q - 1) // 2) != F.one:
                break
        F._ts = (s, t, F.pow(z, t))
    s, t, zt = F._ts
    x = F.pow(a, (t - 1) // 2)
    c, x, b, m = zt, F.mul(x, a), F.mul(F.mul(x, x), a), s
    while b != F.one:
        i, w = 0, b
        while w != F.one:
            w, i = F.mul(w, w), i + 1
        g = c
        for _ in range(m - i - 1):
            g = F.mul(g, g)
        x, c = F.mul(x, g), F.mul(g, g)
        b, m = F.mul(b, c), i
    return x


# ---- the curve y^2 = x^3 + a x + b ------------------------------------------------------------------------------------------
class Curve:
    """points are None (O) or (x, y); the case analysis of curve_mul / curve_double (ecc/curve.c:102-207)"""

    def __init__(self, field, a, b, r):
        self.F, self.a, self.b, self.r = field, a, b, r

    def rhs(self, x):
        F = self.F
        return F.add(F.mul(F.add(F.mul(x, x), self.a), x), self.b)

    def on_curve(self, P):
        return P is None or self.F.mul(P[1], P[1]) == self.rhs(P[0])

    def from_x(self, x):
        y = sqrt(self.F, self.rhs(x))
        return None if y is None else (x, y)

    def neg(self, P):
        return None if P is None else (P[0], self.F.neg(P[1]))

    def dbl(self, P):
        F = self.F
        if P is None or P[1] == F.zero:
            return None
        x, y = P
        xx = F.mul(x, x)
        lam = F.mul(F.add(F.add(F.double(xx), xx), self.a), F.inv(F.double(y)))
        x3 = F.sub(F.mul(lam, lam), F.double(x))
        return (x3, F.sub(F.mul(F.sub(x, x3), lam), y))

    def add(self, P, Q):
        F = self.F
        if P is None:
            return Q
        if Q is None:
            return P
        if P[0] == Q[0]:
            return self.dbl(P) if P[1] == Q[1] else None
        lam = F.mul(F.sub(Q[1], P[1]), F.inv(F.sub(Q[0], P[0])))
        x3 = F.sub(F.sub(F.mul(lam, lam), P[0]), Q[0])
        return (x3, F.sub(F.mul(F.sub(P[0], x3), lam), P[1]))

    def sub(self, P, Q):
        return self.add(P, self.neg(Q))

    def mul(self, k, P, reduce=True):
        """double-and-add from the top bit; k mod r first, as the reference reads a record of Z_r.  reduce=False: the
        integer as it stands -- what include/pbc_hip.h states for element_mul_zn ("scalars may exceed r") and the suite
        pins on points of small order; the two differ only for k >= r on a point outside the order-r subgroup.  The
        batteries judge the library by its header (reduce=False throughout); reduce=True reproduces the fixtures"""
        if reduce:
            k %= self.r
        R = None
        for bit in bin(k)[2:]:
            R = self.dbl(R)
            if bit == "1":
                R = self.add(R, P)
        return R

    def add_many(self, pairs):
        """[P + Q for (P, Q) in pairs] by the same case analysis, the denominators inverted together (Montgomery's trick:
        one inversion of their product) -- in Python the inversion is what a group operation costs"""
        F = self.F
        out, den, idx = [None] * len(pairs), [], []
        for i, (P, Q) in enumerate(pairs):
            if P is None:
                out[i] = Q
            elif Q is None:
                out[i] = P
            elif P[0] != Q[0]:
                den.append(F.sub(Q[0], P[0]))
                idx.append(i)
            elif P[1] == Q[1] and P[1] != F.zero:
                den.append(F.double(P[1]))
                idx.append(i)
        if not den:
            return out
        pre = [den[0]]
        for x in den[1:]:
            pre.append(F.mul(pre[-1], x))
        run = F.inv(pre[-1])
        for n in range(len(den) - 1, -1, -1):
            dinv = F.mul(run, pre[n - 1]) if n else run
            run = F.mul(run, den[n])
            P, Q = pairs[idx[n]]
            if P[0] != Q[0]:
                num = F.sub(Q[1], P[1])
            else:
                xx = F.mul(P[0], P[0])
                num = F.add(F.add(F.double(xx), xx), self.a)
            lam = F.mul(num, dinv)
            x3 = F.sub(F.sub(F.mul(lam, lam), P[0]), Q[0])
            out[idx[n]] = (x3, F.sub(F.mul(F.sub(P[0], x3), lam), P[1]))
        return out

    def mul_batch(self, units, reduce=True):
        """[[k] P for (k, P) in units], k as in mul, by hexadecimal digits from the low end: k = sum d_i 16^i, so
        [k] P = sum over d = 1..15 of d B_d with B_d the sum of the 16^i P whose digit is d.  The units that share a point
        share its chain 16^i P; every level is one add_many, and so is every step of the closing sum
        (B_15) + (B_15 + B_14) + ... -- about 5/9 of the additions of the bit-by-bit ladder on a dense scalar"""
        ks = [k % self.r if reduce else k for k, _ in units]
        chains = {}
        for _, P in units:
            chains.setdefault(P, P)
        B = [[None] * 16 for _ in units]
        levels = (max(ks).bit_length() + 3) // 4 if ks else 0
        for i in range(levels):
            todo = [(j, (k >> (4 * i)) & 15) for j, k in enumerate(ks) if (k >> (4 * i)) & 15]
            for (j, d), R in zip(todo, self.add_many([(B[j][d], chains[units[j][1]]) for j, d in todo])):
                B[j][d] = R
            if i + 1 < levels:
                keys = list(chains)
                for _ in range(4):
                    for P, D in zip(keys, self.add_many([(chains[P], chains[P]) for P in keys])):
                        chains[P] = D
        run, acc = [None] * len(units), [None] * len(units)
        for d in range(15, 0, -1):
            run = self.add_many([(R, b[d]) for R, b in zip(run, B)])
            acc = self.add_many(list(zip(acc, run)))
        return acc

    def mul_many(self, ks, P, reduce=True):
        return self.mul_batch([(k, P) for k in ks], reduce)


class Layout:
    """a point record: x then y, each d coefficients (coefficient 0 first) of fb big-endian bytes; O = zero bytes"""

    def __init__(self, curve, fb):
        self.C, self.F, self.fb = curve, curve.F, fb
        self.length = 2 * fb * curve.F.d

    def elem(self, raw):
        fb, q = self.fb, (self.F.m if self.F.d == 1 else self.F.q)
        return self.F.from_coeffs([int.from_bytes(raw[i * fb:(i + 1) * fb], "big") % q for i in range(self.F.d)])

    def decode(self, rec, zero_is_O=True):
        """record -> point.  Off-curve records are O (curve_from_bytes); the all-zero record is O, or -- zero_is_O false,
        on a curve with b = 0 -- the point (0, 0), as include/pbc_hip.h states per entry point"""
        raw = bytes(rec)
        if zero_is_O and not any(raw):
            return None
        P = (self.elem(raw[:self.length // 2]), self.elem(raw[self.length // 2:]))
        return P if self.C.on_curve(P) else None

    def encode(self, P):
        if P is None:
            return bytes(self.length)
        return b"".join(int(c).to_bytes(self.fb, "big") for v in P for c in self.F.coeffs(v))

    def pack(self, pts):
        return np.frombuffer(b"".join(self.encode(P) for P in pts), np.uint8).reshape(len(pts), self.length).copy()

    def unpack(self, recs, zero_is_O=True):
        return [self.decode(r.tobytes(), zero_is_O) for r in np.ascontiguousarray(recs, np.uint8)]


class Family:
    pass


def param_dict(text):
    out = {}
    for line in text.splitlines():
        f = line.split()
        if len(f) == 2:
            out[f[0]] = f[1] if f[0] == "type" else (int(f[1]) if f[1].lstrip("-").isdigit() else f[1])
    return out


def family(text):
    """parameter text -> .type, .q, .r, .fq, .zr, .g1 / .g2 (Curve), .lay1 / .lay2 (Layout), .fb, .zl"""
    p = param_dict(text)
    S = Family()
    S.type = p["type"]
    S.q = p["p"] if S.type == "a1" else p["q"]
    S.r = p["n"] if S.type == "a1" else p["r"]
    S.fq, S.zr = Fq(S.q), Zr(S.r)
    S.fb, S.zl = (S.q.bit_length() + 7) // 8, (S.r.bit_length() + 7) // 8
    q = S.q
    if S.type in ("a", "a1"):
        S.g1 = S.g2 = Curve(S.fq, 1, 0, S.r)
    elif S.type == "e":
        S.g1 = S.g2 = Curve(S.fq, p["a"] % q, p["b"] % q, S.r)
    elif S.type in ("d", "g"):
        d = p["k"] // 2
        S.g1 = Curve(S.fq, p["a"] % q, p["b"] % q, S.r)
        E = Ext(q, [p["coeff%d" % i] for i in range(d)])
        nqr = p["nqr"] % q
        S.g2 = Curve(E, E.embed(p["a"] * nqr * nqr), E.embed(p["b"] * nqr ** 3), S.r)
    elif S.type == "f":
        S.g1 = Curve(S.fq, 0, p["b"] % q, S.r)
        E = Ext(q, [-p["beta"], 0])
        S.g2 = Curve(E, E.zero, E.from_coeffs([-p["alpha0"] * p["b"], -p["alpha1"] * p["b"]]), S.r)
    else:
        raise ValueError("type " + S.type)
    S.lay1, S.lay2 = Layout(S.g1, S.fb), Layout(S.g2, S.fb)
    return S


# ---- crafted operands -------------------------------------------------------------------------------------------------------
def rbits_of(nbytes):
    """bits of the Montgomery radix of the library's limb form for a modulus of nbytes bytes (test_gpu_soak._rbits)"""
    n_words = -(-(nbytes * 8) // 32)
    if n_words > 16:
        return 28 * 38
    return 29 * (-(-32 * n_words // 29))


def limb_bits(rbits):
    return 29 if rbits % 29 == 0 else 28


def soak_pattern(t, m, rbits):
    """pattern t < 22 of oracle/ref_harness.c soak_pattern in the library's limb width: an integer below m"""
    W = limb_bits(rbits)
    L = rbits // W
    ones = (1 << W) - 1
    if t in (0, 6):
        v = m - 1
    elif t == 1:
        v = m - 2
    elif t in (2, 7):
        v = 1
    elif t == 3:
        v = 2
    elif t == 4:
        v = (m - 1) >> 1
    elif t == 5:
        v = (m + 1) >> 1
    elif t == 8:
        v = (1 << (W * L)) - 1
    elif t in (9, 10, 11):
        v = ones << (W * {9: 0, 10: L // 2, 11: L - 2}[t])
    elif t in (12, 13):
        v = sum(ones << (W * i) for i in range(t - 12, L, 2))
    elif t == 14:
        v = 1 << W
    elif t == 15:
        v = 1 << (W * (L // 2))
    elif t == 16:
        v = 1 << (W * (L - 2))
    elif t == 17:
        v = sum(1 << (W * i + W - 1) for i in range(L))
    elif t == 18:
        v = sum(1 << (W * i) for i in range(L))
    elif t == 19:
        v = (1 << (32 * ((W * L) // 64))) - 1
    elif t == 20:
        v = (1 << (W * (L - 1))) - 1
    else:
        v = (((1 << (W * L)) - 1) >> 1) << 1
    if v >= m:
        v &= (1 << (m.bit_length() - 1)) - 1
    return v


N_PATTERNS = 22


def patterns(m, rbits):
    """[(label, t, mont, v)]: t the pattern number (22 + i for the i-th added row), mont whether v is meant as the
    Montgomery residue (the operand is then v / 2^rbits mod m: operand()); the 22 patterns in both domains, then 2^j and
    m - 2^j for j on every limb boundary below m, in both domains"""
    W = limb_bits(rbits)
    rows = [("p%d" % t, t, soak_pattern(t, m, rbits)) for t in range(N_PATTERNS)]
    t = N_PATTERNS
    for j in range(0, m.bit_length(), W):
        if (1 << j) < m:
            rows += [("2^%d" % j, t, 1 << j), ("m-2^%d" % j, t + 1, m - (1 << j))]
            t += 2
    out, seen = [], set()
    for mont in (False, True):
        for label, t, v in rows:
            x = operand(v, mont, m, rbits)
            if x not in seen:
                seen.add(x)
                out.append((label + ("/R" if mont else ""), t, mont, v))
    return out


def operand(v, mont, m, rbits, bump=0):
    """the field element a pattern row stands for, nudged `bump` upwards in the row's own domain"""
    v = (v + bump) % m
    return v * pow(1 << rbits, -1, m) % m if mont else v


def noncanonical(v, m, nbytes):
    """v + t m with the largest t that fits nbytes bytes"""
    return v + ((1 << (8 * nbytes)) - 1 - v) // m * m


def scalars(r, zl, pow2_rows=True):
    """[(label, k)], k < 2^(8 zl): the suite's edge list first, then structured nibbles (d_i = 2 ((k' >> (4 i + 1)) & 15) - 15
    is the window recoding they aim at), each value also with its lowest bit flipped (even k: [k] P = [k + 1] P - P)"""
    top = 1 << (8 * zl)
    rows = [(str(k) if k < 100 else lab, k) for lab, k in
            [("", 0), ("", 1), ("", 2), ("", 3), ("r-1", r - 1), ("r-2", r - 2), ("r", r), ("2^(8zl)-1", top - 1), ("2^(8zl)-2", top - 2),
             ("", 15), ("", 16), ("", 17)]]
    for nib in range(1, 16):
        v = int("%x" % nib * (2 * zl), 16)
        rows += [("0x%x.." % nib, v), ("0x%x.. mod r" % nib, v % r)]
    rows += [("0x0f0f..", int("0f" * zl, 16)), ("0xf0f0..", int("f0" * zl, 16)), ("0x7f..f", top // 2 - 1), ("0x80..0", top // 2),
             ("0x80..01", top // 2 + 1)]
    if pow2_rows:
        for i in range(2 * zl):
            for j in (4 * i, 4 * i + 1):
                rows += [("2^%d" % j, 1 << j), ("2^%d+1" % j, (1 << j) + 1), ("2^%d-1" % j, (1 << j) - 1)]
    rows += [("r+1", r + 1), ("r+2", r + 2), ("(r-1)/2", (r - 1) // 2), ("(r+1)/2", (r + 1) // 2), ("2r-1", 2 * r - 1), ("2r+1", 2 * r + 1)]
    out, seen = [], set()
    for flip in (0, 1):
        for label, k in rows:
            k ^= flip
            if 0 <= k < top and k not in seen:
                seen.add(k)
                out.append((label + ("^1" if flip else ""), k))
    return out


# Operands that drive fp_inv's safegcd loop deep: for each F_q battery set, the integer g (the Montgomery residue the
# divsteps start from, f = q) with the largest divstep count a bit-flipping hill climb found, and that count.
#
# What they can and cannot show.  fp_inv runs ceil(B(32 N) / 30) batches of 30 divsteps, B(b) = (45907 b + 26313) div 19929
# the proven bound for b-bit inputs (2.30 per bit).  Uniform operands need 2.02 bits(q) divsteps, within a few per cent; the
# rows below 2.05 - 2.11 bits(q).  Batches run / batches B(bits(q)) needs / batches the row below needs:
#     a 40/40/36   d159 13/13/12   d278027-190-181 15/15/14   d201 18/16/14   f_256 20/20/18   a_160_256 20/20/18
#     a_160_500 40/39/35   a_224_768 59/59/53   a1 82/80/71   e 79/79/70   a_160_1024 79/79/70   g149 13/12/11
# On d201, a_160_500, a1 and g149 the last batch is idle on every operand, by the bound itself (q is shorter than 32 N bits).
# On the other eight the bound allows an operand that needs the last batch, but it is a bound over all pairs (f, g); with
# f = q fixed no such g is known, the search found none, and a loop one batch short is not told apart by these rows.
# They tell apart a loop two batches short on d159 and d278027-190-181, and 3 - 10 short on the rest -- a batch or two
# earlier than uniform operands do.
DEEP_DIVSTEPS = {
    "a": (1059, int(
        "965b109fc2ef230ae88d759693203a773e4ce22c2645b5646a3c8b1989f19bd53bcc44b92fe1b34b04941aa1da739fc6ede8"
        "2ca7932adf425d65620f787248f2", 16)),
    "d159": (334, int(
        "4b0ff4c8f82d41a5dde9e257140957c647c2efd7", 16)),
    "d278027-190-181": (398, int(
        "269b1fa5d9d4f4b232ece850ece19d1a0baa64675c7dddb3", 16)),
    "d201": (420, int(
        "143245e53b13229c019a1ef97eddde5c043c25f56e8662a252b", 16)),
    "f_256": (530, int(
        "cf176f4d268952d6af3cf93b0ca1e9b749df11a33c38a75697849ba9ba79a78", 16)),
    "a_160_256": (528, int(
        "181f1acd05275d2c4c601cb99d6a55f9cb55ddc4bdfbb60c572c1736b3d952bc", 16)),
    "a_160_500": (1031, int(
        "346392892f7c04f976fbbe1f755912355dbb4c76e630cf3f28295ccb2ce7b96bb555ca386ff607f4ae2804876b60aefb6aa3"
        "0fd01701a56acfbba69249aa2", 16)),
    "a_224_768": (1581, int(
        "2b027418e904f9b1711f5e8b8dadf199254c8aa5c643e8258032c5b9f61f98a81beac7fe030da7d0ad7f3f2e04cf8ef18c0b"
        "8b83d82a881b2c671ce95f31393ecb6df89ff0de22ecc932a155455929bb606a0f01a3682d26e6607d493bed6c0", 16)),
    "a1": (2116, int(
        "935b5698b8fb58fc88b72ba01915bbd9beb10bbff00f1d8e4324c63f51149e819133a9f8ad398cc805d22965e6c9e5ea022d"
        "cb7a43d57a2d2dedce05194d694827dce57576fd7e5f4296aa9f4e47c4ddb9abdc01a64a551a3dbf81b652219e4d68da675f"
        "331a9372814a69ba21209c356b00fea89592050c052321fcbe59acab1d", 16)),
    "e": (2091, int(
        "501f6b9303fe49dec9459376a8b8b40b99bfab701fb71b962d4d4d689b621d5feeeb0212593168666041bf00ea2380a2a142"
        "25ac31f128347ba22d44af5b5075c6716796937480026bb7406bb13084f9cc381c95a28269f217f05e1c3ce7b3879027d689"
        "b5ac61a6d9cc2fa7b183e5790e3a4583db250e8059352389e278d96", 16)),
    "a_160_1024": (2092, int(
        "10641d2cb631b98957b31a7953c06284a2783ebdcccf4d33983c29f34d65545b4f386c0e927ad3b9b66be43183ddb0e707fa"
        "15f95164c7e5e18c01cf35fc33be78ce6c50483a8ae89fd6f83f91eca096ef97911f717138747b289f465314c3487aa899cb"
        "85424b8ff0c9f145468fc9b8853d477895203bd6c3673735434be699", 16)),
    "g149": (314, int(
        "1559639edc666553da7e4c2a7355a567cf6ecf", 16)),
}


def divsteps(f, g):
    """the number of half-delta divsteps (pbc_amd/csrc/fp.cuh inv_divsteps30) until g = 0"""
    zeta, n = -1, 0
    while g:
        if g & 1:
            if zeta < 0:
                zeta, f, g = -zeta - 2, g, (g - f) >> 1
            else:
                zeta, g = zeta - 1, (g + f) >> 1
        else:
            zeta, g = zeta - 1, g >> 1
        n += 1
    return n


# ---- batteries: inputs and expected bytes, shared by the CPU twin and the GPU tests ------------------------------------------------
FIXTURE_OF = {"a": "a_rand32.vec", "d159": "d_rand32.vec", "f": "f_rand16.vec", "g149": "g149_rand16.vec", "d201": "d201_rand12.vec",
              "e": "e_rand6.vec", "a1": "a1_rand6.vec", "a1_200": "a1_200_rand6.vec", "f_256": "f_256_rand4.vec",
              "a_160_256": "a_160_256_rand6.vec"}
HIP_KEY = {"d159": "d"}                                        # the key of the hips / oracles / sims fixtures
POW2_EVERY = {("d201", 2): 3}                                  # sizing: (name, group) -> every n-th 2^j row of the scalar list


def fam(name):
    from conftest import _param
    return _family_cached(_param(name))


@functools.lru_cache(maxsize=None)
def _family_cached(text):
    return family(text)


def _ints_to_recs(vals, nbytes):
    return np.frombuffer(b"".join(int(v).to_bytes(nbytes, "big") for v in vals), np.uint8).reshape(len(vals), nbytes).copy()


def ragged(n):
    """the next length of the form 64 k + 1"""
    return -(-(n - 1) // 64) * 64 + 1 if n > 1 else 1


def _rng(name, salt):
    return np.random.default_rng([salt] + list(name.encode()))


def _rand_below(rng, m):
    return int.from_bytes(rng.bytes((m.bit_length() + 7) // 8 + 8), "big") % m


def _modular_battery(R, m, nbytes, name, salt, binary_ops, unary_ops, skip_zero_b_ops, skip_zero_a_ops, usable, extra=()):
    """pairs (A, B): every pattern x a 12-element subset, (A, A), (A, m - A), padded with random pairs to 64 k + 1"""
    rbits = rbits_of(nbytes)
    pats = [operand(v, mont, m, rbits) for _, _, mont, v in patterns(m, rbits)]
    pats = [x for x in pats if usable(x)] + list(extra)
    by = {lab: operand(v, mont, m, rbits) for lab, _, mont, v in patterns(m, rbits)}
    W = limb_bits(rbits)
    subset = [by[k] for k in ("p0", "p2", "p3", "p5", "p8/R", "p12/R", "p13/R", "p17/R", "p20/R", "p21/R", "p0/R", "m-2^%d" % W) if k in by]
    subset = [x for x in subset if usable(x)]
    for x in pats:                                               # (a1's Z_r: a label that shares a factor with n is replaced
        if len(subset) < 12 and x not in subset:                 #  by the next pattern that does not)
            subset.append(x)
    assert len(set(subset)) == 12, (name, len(set(subset)))
    pairs = [(a, b) for a in pats for b in subset] + [(a, a) for a in pats] + [(a, (m - a) % m) for a in pats]
    rng = _rng(name, salt)
    while len(pairs) != ragged(len(pairs)):
        a, b = _rand_below(rng, m), _rand_below(rng, m)
        if usable(a) and usable(b):
            pairs.append((a, b))
    A, B = _ints_to_recs([a for a, _ in pairs], nbytes), _ints_to_recs([b for _, b in pairs], nbytes)
    cases = []                                                   # (op, rows kept, expected records)
    for op in sorted(binary_ops + unary_ops):
        keep = [i for i, (a, b) in enumerate(pairs)
                if not (op in skip_zero_a_ops and a % m == 0) and not (op in skip_zero_b_ops and b % m == 0)]
        want = [R.op(op, pairs[i][0], pairs[i][1] if op in binary_ops else None) for i in keep]
        cases.append((op, np.array(keep), _ints_to_recs(want, nbytes)))
    return A, B, cases, pats


@functools.lru_cache(maxsize=None)
def battery_fq(name):
    """-> A, B, [(op, rows, expected)], NA, [(op, rows, expected)]: NA = every pattern, and 0, as the record v + t q (op 0:
    NA * NA; op 3 on the rows that are not 0 mod q)"""
    S = fam(name)
    deep = operand(DEEP_DIVSTEPS[name][1], True, S.q, rbits_of(S.fb))      # the named case "deep divsteps"
    A, B, cases, pats = _modular_battery(S.fq, S.q, S.fb, name, 1, [0, 1, 2], [3, 4, 5, 6], [], [3], lambda x: True, [deep])
    nc = pats + [0]                                               # (0 as the record t q: op 0 only)
    NA = _ints_to_recs([noncanonical(x, S.q, S.fb) for x in nc], S.fb)
    inv_rows = np.array([i for i, x in enumerate(nc) if x % S.q])
    nc_cases = [(0, np.arange(len(nc)), _ints_to_recs([x * x % S.q for x in nc], S.fb)),
                (3, inv_rows, _ints_to_recs([S.fq.inv(nc[i]) for i in inv_rows], S.fb))]
    return A, B, cases, NA, nc_cases


@functools.lru_cache(maxsize=None)
def battery_zr(name):
    """Z_r: the patterns on the modulus r (a1: n, where operands sharing a factor with n are left out -- .dropped says how
    many of the pattern set that removes)"""
    S = fam(name)
    usable = (lambda x: math.gcd(x, S.r) == 1) if S.type == "a1" else (lambda x: True)
    A, B, cases, pats = _modular_battery(S.zr, S.r, S.zl, name, 2, [0, 1, 2, 7], [3, 4, 5, 6], [7], [3], usable)
    total = len(patterns(S.r, rbits_of(S.zl)))
    return A, B, cases, total - len(pats), total


def crafted_points(name, group):
    """[(label, point)] of the whole curve: x follows each pattern row, nudged upwards in the row's domain until a point
    exists; on a twist once with every coefficient of x carrying the pattern and once with the first alone; rows with an
    odd pattern number give -P"""
    return _crafted_points(name, group)


@functools.lru_cache(maxsize=None)
def _crafted_points(name, group):
    S = fam(name)
    C = S.g1 if group == 1 else S.g2
    F, rbits = C.F, rbits_of(S.fb)
    out = []
    for label, t, mont, v in patterns(S.q, rbits):
        for sparse in ((False, True) if F.d > 1 else (False,)):
            bump = 0
            while True:
                x0 = operand(v, mont, S.q, rbits, bump)
                rest = 0 if sparse else operand(v, mont, S.q, rbits)
                x = x0 if F.d == 1 else F.from_coeffs([x0] + [rest] * (F.d - 1))
                P = C.from_x(x)
                if P is not None and P != (F.zero, F.zero):
                    break
                bump += 1
            out.append((label + ("/first" if sparse else ""), C.neg(P) if t & 1 else P))
    return out


def _fixture_points(name, group):
    from conftest import golden
    v = golden(FIXTURE_OF[name])
    return v.g1 if group == 1 else v.g2


@functools.lru_cache(maxsize=None)
def battery_law(name, group):
    """-> A, B, {"add" | "sub" | "neg" | "double": expected}: every crafted point with a fixture point, itself, its negative
    and O (on both sides); the all-zero record is O here"""
    S = fam(name)
    C, lay = (S.g1, S.lay1) if group == 1 else (S.g2, S.lay2)
    fix = lay.unpack(_fixture_points(name, group))
    pa, pb = [], []
    for i, (_, P) in enumerate(crafted_points(name, group)):
        R = fix[i % len(fix)]
        pa += [P, R, P, P, P, None]
        pb += [R, P, P, C.neg(P), None, P]
    rng = _rng(name, 3 + group)
    while len(pa) != ragged(len(pa)):
        pa.append(fix[int(rng.integers(len(fix)))])
        pb.append(fix[int(rng.integers(len(fix)))])
    want = {"add": lay.pack([C.add(a, b) for a, b in zip(pa, pb)]), "sub": lay.pack([C.sub(a, b) for a, b in zip(pa, pb)]),
            "neg": lay.pack([C.neg(a) for a in pa]), "double": lay.pack([C.dbl(a) for a in pa])}
    return lay.pack(pa), lay.pack(pb), want


REDUCED_SCALARS = ("e", "a1", "a1_200")                        # 1000-bit fields: every nibble pattern, no 2^j rows


GROUPS = (1, 2)


def scalar_rows(name, pow2_every=1):
    """scalars(r, zl) of a parameter set; pow2_every > 1 keeps every pow2_every-th of the 2^j rows (sizing: nothing else is thinned)"""
    S = fam(name)
    out, seen = [], 0
    for lab, k in scalars(S.r, S.zl, pow2_rows=name not in REDUCED_SCALARS):
        if lab.startswith("2^") and not lab.startswith("2^("):
            seen += 1
            if seen % pow2_every:
                continue
        out.append((lab, k))
    return out


def whole_curve_scalars(name):
    """the 16 scalars that meet every crafted whole-curve point: all below r, where the reference's reading of a record
    (mod r) and the library's (the integer as it stands, include/pbc_hip.h) are the same thing on any point"""
    S = fam(name)
    r = S.r
    nib = lambda x: int("%x" % x * (2 * S.zl), 16) % r
    ks = [1, 2, 3, 15, 16, 17, r - 1, r - 2, nib(1), nib(7), nib(8), nib(15), (r - 1) // 2, (r + 1) // 2, nib(15) ^ 1, nib(5) ^ 1]
    assert len(set(ks)) == 16 and all(0 < k < r for k in ks)
    return ks


def battery_mul(name, group, pow2_every=1):
    """_battery_mul; on the 1000-bit symmetric sets G2 is G1 (one curve, the same fixture points), and group 2 takes group 1's
    batch through its own entry point"""
    return _battery_mul(name, 1 if name in REDUCED_SCALARS else group, pow2_every)


@functools.lru_cache(maxsize=None)
def _battery_mul(name, group, pow2_every):
    """-> points, scalars, expected for element_mul_zn: every scalar of scalars(r, zl) on a fixture point (of the order-r
    subgroup on G1; G2 of types d, f, g carries no cofactor in the reference, so its fixture points lie on the whole twist
    and a scalar >= r is multiplied as it stands: Curve.mul reduce=False), the 16 whole_curve_scalars on every crafted
    point, the two kinds of rows interleaved"""
    S = fam(name)
    C, lay = (S.g1, S.lay1) if group == 1 else (S.g2, S.lay2)
    fix = lay.unpack(_fixture_points(name, group))
    rows = scalar_rows(name, pow2_every)
    per = [[] for _ in fix]
    for i, (_, k) in enumerate(rows):
        per[i % len(fix)].append(k)
    sub = [(P, k) for P, ks in zip(fix, per) for k in ks]
    sub = [(P, k, R) for (P, k), R in zip(sub, C.mul_batch([(k, P) for P, k in sub], reduce=False))]
    whole = [(P, k) for _, P in crafted_points(name, group) for k in whole_curve_scalars(name)]
    whole = [(P, k, R) for (P, k), R in zip(whole, C.mul_batch([(k, P) for P, k in whole], reduce=False))]
    units = []
    for i in range(max(len(sub), len(whole))):                   # interleave: a wavefront mixes flagged and unflagged lanes
        units += sub[i:i + 1] + whole[i:i + 1]
    rng = _rng(name, 7 + group)
    pad = []
    while len(units) + len(pad) != ragged(len(units)):
        pad.append((fix[int(rng.integers(len(fix)))], _rand_below(rng, S.r)))
    units += [(P, k, R) for (P, k), R in zip(pad, C.mul_batch([(k, P) for P, k in pad], reduce=False))]
    return lay.pack([u[0] for u in units]), _ints_to_recs([u[1] for u in units], S.zl), lay.pack([u[2] for u in units])


@functools.lru_cache(maxsize=None)
def battery_multi(name, group):
    """-> [A1, A2, A3], [N1, N2, N3], expected pow2, expected pow3: every base takes a structured scalar (the nibble and
    edge rows; no 2^j rows); rows with A2 = A1, A2 = -A1 with equal scalars, one base O; the all-zero record is O"""
    S = fam(name)
    C, lay = (S.g1, S.lay1) if group == 1 else (S.g2, S.lay2)
    fix = lay.unpack(_fixture_points(name, group))
    ks = [k for _, k in scalars(S.r, S.zl, pow2_rows=False)]
    ks = ks[:len(ks) // 2]                                        # (the rows with the lowest bit flipped come back as N2 below)
    n = len(ks)
    units = []
    for i, k in enumerate(ks):
        a1, a2, a3 = fix[i % len(fix)], fix[(i + 1) % len(fix)], fix[(i + 2) % len(fix)]
        n1, n2, n3 = k, ks[(i * 7 + 3) % n] ^ 1, ks[(i * 11 + 5) % n]
        if i % 8 == 1:
            a2 = a1
        elif i % 8 == 3:
            a2, n2 = C.neg(a1), n1
        elif i % 8 == 5:
            a2 = None
        elif i % 8 == 7:
            a1 = None
        units.append((a1, a2, a3, n1, n2, n3))
    while len(units) != ragged(len(units)):
        units.append(units[len(units) % n][1:3] + units[len(units) % n][:1] + units[(len(units) * 3) % n][3:])
    m = [C.mul_batch([(u[3 + j], u[j]) for u in units], reduce=False) for j in range(3)]
    p2 = C.add_many(list(zip(m[0], m[1])))
    p3 = C.add_many(list(zip(p2, m[2])))
    bases = [lay.pack([u[j] for u in units]) for j in range(3)]
    zs = [_ints_to_recs([u[3 + j] for u in units], S.zl) for j in range(3)]
    return bases, zs, lay.pack(p2), lay.pack(p3)


def battery_gt(name):
    """-> pairing values (the fixture's), structured scalars: element_pow_zn on GT; the expected bytes are the oracle's"""
    from conftest import golden
    S = fam(name)
    v = golden(FIXTURE_OF[name])
    rows = scalar_rows(name)
    n = ragged(len(rows))
    ks = [rows[i % len(rows)][1] for i in range(n)]
    return v.gt[np.arange(n) % v.n], _ints_to_recs(ks, S.zl)
