"""Test helper: an independent Python restatement of the engine's KeyGenerator / Encryptor.

Streams: sub(call, role, i, j) = BLAKE2Xb(<4Q call role i j>, key = seed, 64 bytes); a sub-stream is SEAL's
Blake2xbPRNG on that value (seal_format.Blake2xbStream, pure Python; or, for the larger cases, buffers from the
library's host seal_blake2xb, which test_seal_format.py pins to the pure-Python one).  The samplers run in Python
integers.  NTTs, the Galois permutation and the rescale of a data prime come from the CPU oracle; the division by the
special prime is done here in Python integers between the oracle's ntt_inv / ntt_fwd."""
import struct

import numpy as np

import seal_format as sf

M64 = (1 << 64) - 1
CALL_SECRET, CALL_PUBLIC, CALL_RELIN, CALL_GALOIS, CALL_SYM, CALL_ASYM = 1, 2, 3, 4, 5, 6
ROLE_A, ROLE_E, ROLE_T = 1, 2, 3
CBD_MAX = 21


class LibStream:
    """Blake2xbStream's interface over the library's host BLAKE2Xb (no device)."""

    def __init__(self, hecdna, seed: bytes):
        self.h, self.seed, self.counter, self.buf = hecdna, seed, 0, b""

    def take(self, n):
        while len(self.buf) < n:
            self.buf += self.h.seal_blake2xb(struct.pack("<Q", self.counter), self.seed, 4096)
            self.counter += 1
        out, self.buf = self.buf[:n], self.buf[n:]
        return out


class Streams:
    def __init__(self, hecdna=None):
        self.h = hecdna  # None: everything in pure Python

    def sub(self, seed: bytes, call, role, i, j) -> bytes:
        data = struct.pack("<4Q", call, role, i, j)
        return self.h.seal_blake2xb(data, seed, 64) if self.h else sf.blake2xb(data, seed, 64)

    def open(self, sub_seed: bytes):
        return LibStream(self.h, sub_seed) if self.h else sf.Blake2xbStream(sub_seed)


def sample_uniform(stream, moduli, N, stats=None):
    """SEAL sample_poly_uniform -> u64[len(moduli)][N]; stats (a dict) receives per limb the redrawn words and the
    total of redraws that were themselves redrawn."""
    nl = len(moduli)
    words = struct.unpack("<%dQ" % (nl * N), stream.take(8 * nl * N))
    out = np.zeros((nl, N), dtype=np.uint64)
    for j, q in enumerate(moduli):
        mm = M64 - M64 % q - 1
        first = again = 0
        for i in range(N):
            v = words[j * N + i]
            k = 0
            while v >= mm:
                v = struct.unpack("<Q", stream.take(8))[0]
                k += 1
            first += k > 0
            again += max(0, k - 1)
            out[j, i] = v % q
        if stats is not None:
            stats.setdefault("first", []).append(first)
            stats["again"] = stats.get("again", 0) + again
    return out


def sample_ternary(stream, N):
    """the uniform sampler with the modulus 3 over N words; coefficient (v mod 3) - 1"""
    return [int(v) - 1 for v in sample_uniform(stream, [3], N)[0]]


def sample_cbd(stream, N):
    b = stream.take(6 * N)
    pc = lambda x: bin(x).count("1")
    return [pc(b[6 * i]) + pc(b[6 * i + 1]) + pc(b[6 * i + 2] & 0x1F)
            - pc(b[6 * i + 3]) - pc(b[6 * i + 4]) - pc(b[6 * i + 5] & 0x1F) for i in range(N)]


def obj(a):
    return np.asarray(a).astype(object)


def u64(a):
    return np.array(a, dtype=np.uint64)


class Ref:
    def __init__(self, o, streams: Streams):
        self.o, self.st = o, streams
        self.N, self.K, self.L = o.N, o.K, o.L
        self.q = [int(x) for x in o.moduli]

    def ntt_signed(self, coeffs, nl):
        """signed coefficients -> their residues on primes 0 .. nl - 1, NTT form, u64[nl][N]"""
        return np.stack([self.o.ntt_fwd(j, u64([c % self.q[j] for c in coeffs])) for j in range(nl)])

    def secret(self, seed):
        t = sample_ternary(self.st.open(self.st.sub(seed, CALL_SECRET, ROLE_T, 0, 0)), self.N)
        return self.ntt_signed(t, self.K)

    def rlwe(self, s, nl, seed_a, seed_e, add=None, stats=None):
        """encrypt_zero_symmetric over primes 0 .. nl - 1: (c0, c1) = (-(a s + NTT(e)) (+ add), a)"""
        a = sample_uniform(self.st.open(seed_a), self.q[:nl], self.N, stats)
        e = self.ntt_signed(sample_cbd(self.st.open(seed_e), self.N), nl)
        c0 = np.zeros((nl, self.N), dtype=np.uint64)
        for j in range(nl):
            x = (-(obj(a[j]) * obj(s[j]) + obj(e[j]))) % self.q[j]
            if add is not None:
                x = (x + obj(add[j])) % self.q[j]
            c0[j] = u64(x)
        return c0, a

    def public(self, s, seed):
        c0, c1 = self.rlwe(s, self.K, self.st.sub(seed, CALL_PUBLIC, ROLE_A, 0, 0),
                           self.st.sub(seed, CALL_PUBLIC, ROLE_E, 0, 0))
        return np.stack([c0, c1])

    def kswitch(self, s, newkey, seed, call, tag, stats=None):
        """generate_one_kswitch_key -> u64[L][2][K][N]"""
        P = self.q[self.K - 1]
        out = np.zeros((self.L, 2, self.K, self.N), dtype=np.uint64)
        for J in range(self.L):
            c0, c1 = self.rlwe(s, self.K, self.st.sub(seed, call, ROLE_A, J, tag),
                               self.st.sub(seed, call, ROLE_E, J, tag), stats=stats)
            c0[J] = u64((obj(c0[J]) + (P % self.q[J]) * obj(newkey[J])) % self.q[J])
            out[J, 0], out[J, 1] = c0, c1
        return out

    def relin(self, s, seed, stats=None):
        s2 = np.stack([u64(obj(s[j]) * obj(s[j]) % self.q[j]) for j in range(self.K)])
        return self.kswitch(s, s2, seed, CALL_RELIN, 0, stats)

    def galois(self, s, elt, seed):
        return self.kswitch(s, self.o.apply_galois_ntt(s, elt).reshape(self.K, self.N), seed, CALL_GALOIS, elt)

    def encrypt_symmetric(self, s, pt, seed, v):
        l = pt.shape[0]
        c0, c1 = self.rlwe(s, l, self.st.sub(seed, CALL_SYM, ROLE_A, v, 0), self.st.sub(seed, CALL_SYM, ROLE_E, v, 0),
                           add=pt)
        return np.stack([c0, c1])

    def divide_round(self, t, last):
        """RNSTool::divide_and_round_q_last_ntt over t u64[last + 1][N] (limb i on prime i) in Python integers"""
        qL = self.q[last]
        h = qL >> 1
        y = [int(x) for x in self.o.ntt_inv(last, t[last])]
        out = np.zeros((last, self.N), dtype=np.uint64)
        for i in range(last):
            qi = self.q[i]
            corr = self.o.ntt_fwd(i, u64([(((x + h) % qL) % qi - h % qi) % qi for x in y]))
            out[i] = u64((obj(t[i]) - obj(corr)) * pow(qL, -1, qi) % qi)
        return out

    def encrypt(self, orc, pk, pt, scale, seed, v):
        """encrypt_zero_internal (asymmetric) at the level above + divide-and-round + add plain -> u64[2][l][N]"""
        l = pt.shape[0]
        nl = l + 1  # primes 0 .. l; for l = L prime l is the special prime
        u = self.ntt_signed(sample_ternary(self.st.open(self.st.sub(seed, CALL_ASYM, ROLE_T, v, 0)), self.N), nl)
        t = np.zeros((2, nl, self.N), dtype=np.uint64)
        for k in range(2):
            e = self.ntt_signed(sample_cbd(self.st.open(self.st.sub(seed, CALL_ASYM, ROLE_E, v, k)), self.N), nl)
            for j in range(nl):
                t[k, j] = u64((obj(u[j]) * obj(pk[k][j]) + obj(e[j])) % self.q[j])
        if l < self.L:  # a data prime: the oracle's rescale_to_next
            c = self.o.rescale(orc.Ct(t, float(scale) * self.q[l])).data
            assert np.array_equal(c[0], self.divide_round(t[0], l))  # and the integer restatement agrees with it
        else:
            c = np.stack([self.divide_round(t[k], l) for k in range(2)])
        c = c.copy()
        for j in range(l):
            c[0, j] = u64((obj(c[0, j]) + obj(pt[j])) % self.q[j])
        return c

    # ---- structure: the noise polynomial a sample hides
    def noise_of(self, c0, c1, s, nl, sub=None):
        """INTT_j(c0 + c1 s - sub) per limb j < nl as centred integers -> list of nl lists"""
        out = []
        for j in range(nl):
            q = self.q[j]
            x = (obj(c0[j]) + obj(c1[j]) * obj(s[j])) % q
            if sub is not None:
                x = (x - obj(sub[j])) % q
            y = [int(w) for w in self.o.ntt_inv(j, u64(x))]
            out.append([w - q if w > q // 2 else w for w in y])
        return out
