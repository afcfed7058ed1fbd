"""An integer model of the four curves with fused fixed-base kernels (ED25519, ED448, NIST256, SECP256K1): test infrastructure,
Python integers and nothing else.  It judges GPU results independently of every GPU path and of the CPU oracle.

The plain model is affine addition and double-and-add:

  m = model("ED25519")
  m.add(P, Q), m.mul(k, P)        points are (x, y) tuples of integers; None is the point at infinity (the neutral element)
  m.affine_bytes(e, P)            e*P as two big-endian records of m.nbytes; None leaves as (0, 1), as ecnXXXget gives it
  m.G, m.q, m.p, m.nbytes         generator, prime group order, field prime, record length

tests/test_curve_model_cpu.py pins it to every `mul` record of the curve fixtures under tests/golden/ and to q*G = (0, 1).

m.base_bytes(scalars) gives the records of e*G for many scalars at a fraction of the cost (a table of the multiples d * 2^(8 i) * G
built with the affine addition above, projective accumulation, one inversion per scalar); the same CPU test pins it to the plain
model.  The constants come from modarith_amd.curves, never from here.
"""
from modarith_amd import curves

EDWARDS = ("ED25519", "ED448")
WEIERSTRASS = ("NIST256", "SECP256K1")
_MODELS = {}


class _Model:
    def __init__(self, name, p, q, G, nbytes):
        self.name, self.p, self.q, self.G, self.nbytes = name, p, q, G, nbytes
        self._table = None

    def mul(self, k, P):
        """k*P by double-and-add from the top bit (k >= 0, not reduced: the kernels take any record)"""
        R = None
        for bit in bin(k)[2:] if k else "":
            R = self.add(R, R)
            if bit == "1":
                R = self.add(R, P)
        return R

    def export(self, P):
        x, y = (0, 1) if P is None else P
        return x.to_bytes(self.nbytes, "big"), y.to_bytes(self.nbytes, "big")

    def affine_bytes(self, e, P):
        return self.export(self.mul(e, P))

    # ---- many multiples of the generator
    def _base_table(self):
        """table[i][d] = d * 2^(8 i) * G for d = 1..255 (affine; table[i][0] unused), by the affine addition"""
        if self._table is None:
            rows, B = [], self.G
            for _ in range(self.nbytes):
                row, T = [None, B], B
                for _ in range(254):
                    T = self.add(T, B)
                    row.append(T)
                rows.append(row)
                B = self.add(T, B)
            self._table = rows
        return self._table

    def base_point(self, e):
        """e*G as an affine point or None, 0 <= e < 2^(8 nbytes)"""
        table, acc, i = self._base_table(), self.proj_zero(), 0
        while e:
            if e & 255:
                acc = self.proj_add_affine(acc, table[i][e & 255])
            e >>= 8
            i += 1
        return self.proj_affine(acc)

    def base_bytes(self, scalars):
        return [self.export(self.base_point(e)) for e in scalars]


class _Edwards(_Model):
    """a x^2 + y^2 = 1 + d x^2 y^2 with a square and d not: the addition law is complete, the neutral element is (0, 1)"""
    def __init__(self, name):
        c = curves.curve(name)
        p = c.fp.p
        super().__init__(name, p, c.order, (c.gx % p, c.gy % p), c.fp.nbytes)
        self.a, self.d = c.a % p, c.d % p

    def add(self, P, Q):
        p = self.p
        (x1, y1), (x2, y2) = P or (0, 1), Q or (0, 1)
        t = self.d * x1 * x2 * y1 * y2 % p
        x3 = (x1 * y2 + y1 * x2) * pow(1 + t, -1, p) % p
        y3 = (y1 * y2 - self.a * x1 * x2) * pow(1 - t, -1, p) % p
        return None if (x3, y3) == (0, 1) else (x3, y3)

    # projective (X : Y : Z), x = X / Z, y = Y / Z (Bernstein, Birkner, Joye, Lange, Peters 2008: complete for these curves)
    def proj_zero(self):
        return (0, 1, 1)

    def proj_add_affine(self, A, Q):
        p = self.p
        X1, Y1, Z1 = A
        x2, y2 = Q or (0, 1)
        B = Z1 * Z1 % p
        C, D = X1 * x2 % p, Y1 * y2 % p
        E = self.d * C * D % p
        F, G = B - E, B + E
        return (Z1 * F * ((X1 + Y1) * (x2 + y2) - C - D) % p, Z1 * G * (D - self.a * C) % p, F * G % p)

    def proj_affine(self, A):
        zi = pow(A[2], -1, self.p)
        P = (A[0] * zi % self.p, A[1] * zi % self.p)
        return None if P == (0, 1) else P


class _Weierstrass(_Model):
    """y^2 = x^3 + a x + b of prime order: chord and tangent, with the point at infinity and P + (-P) spelled out"""
    def __init__(self, name):
        c = curves.wcurve(name)
        p = c.fp.p
        super().__init__(name, p, c.order, (c.gx % p, c.gy % p), c.fp.nbytes)
        self.a, self.b = c.a % p, c.b % p

    def add(self, P, Q):
        p = self.p
        if P is None:
            return Q
        if Q is None:
            return P
        (x1, y1), (x2, y2) = P, Q
        if x1 == x2:
            if (y1 + y2) % p == 0:
                return None
            lam = (3 * x1 * x1 + self.a) * pow(2 * y1, -1, p) % p
        else:
            lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
        x3 = (lam * lam - x1 - x2) % p
        return (x3, (lam * (x1 - x3) - y1) % p)

    # Jacobian (X : Y : Z), x = X / Z^2, y = Y / Z^3; Z = 0 is the point at infinity
    def proj_zero(self):
        return (1, 1, 0)

    def proj_add_affine(self, A, Q):
        p = self.p
        X1, Y1, Z1 = A
        if Q is None:
            return A
        x2, y2 = Q
        if Z1 == 0:
            return (x2, y2, 1)
        Z2 = Z1 * Z1 % p
        H, R = (x2 * Z2 - X1) % p, (y2 * Z2 * Z1 - Y1) % p
        if H == 0:
            if R:
                return (1, 1, 0)                                   # A = -Q
            M, S = (3 * X1 * X1 + self.a * Z2 * Z2) % p, 4 * X1 * Y1 * Y1 % p        # A = Q: the tangent
            X3 = (M * M - 2 * S) % p
            return (X3, (M * (S - X3) - 8 * pow(Y1, 4, p)) % p, 2 * Y1 * Z1 % p)
        H2 = H * H % p
        H3, V = H * H2 % p, X1 * H2 % p
        X3 = (R * R - H3 - 2 * V) % p
        return (X3, (R * (V - X3) - Y1 * H3) % p, Z1 * H % p)

    def proj_affine(self, A):
        if A[2] == 0:
            return None
        zi = pow(A[2], -1, self.p)
        z2 = zi * zi % self.p
        return (A[0] * z2 % self.p, A[1] * z2 * zi % self.p)


def model(name):
    name = name.upper()
    if name not in _MODELS:
        _MODELS[name] = (_Edwards if name in EDWARDS else _Weierstrass)(name)
    return _MODELS[name]


def affine_bytes(name, e, P):
    """(x, y) of e*P on the named curve as big-endian records; P = None is the point at infinity"""
    return model(name).affine_bytes(e, P)
