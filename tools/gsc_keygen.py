#!/usr/bin/env python3
"""Key generation for the reference's circuits with the product's Groth16 Setup (gsc_setup) — what `go run keygen.go` does with
gnark (reference keygen.go:341-352, :380-391, :419-430) for the R1CS files it ships.  Toxic waste comes from the OS CSPRNG.

  python tools/gsc_keygen.py <r1cs file> <pk out> <vk out>
e.g. python tools/gsc_keygen.py r1cs.aes128 pk.aes128 vk.aes128      (needs a GPU: the group elements are computed there)

Key ceremony, second phase: every party re-randomises delta of the pair it was handed and passes the result
on; anyone checks every link with the published records before the final pair is loaded.

  python tools/gsc_keygen.py --contribute PK VK --out-dir D
      writes D/<name of PK>, D/<name of VK> and D/contribution.record (224 bytes); the secret comes from the OS CSPRNG and is gone when the
      command returns
  python tools/gsc_keygen.py --verify-contribution PREV_PK PREV_VK NEXT_PK NEXT_VK RECORD
      prints ACCEPTED (exit status 0) or REFUSED (exit status 1; the library's line above it names the rule that failed)

Key ceremony, first phase: a key whose tau, alpha and beta nobody knows starts from a powers file (this project's
own format, include/libprove.h — not snarkjs' .ptau, not gnark's mpcsetup).  The file starts at tau = alpha = beta = 1 and every party
multiplies the scalars by secrets of its own; anyone checks every link, from the starting file on, with the published records.

  python tools/gsc_keygen.py --srs-initial L OUT
      writes the starting file for N = 2^L (no GPU needed; deterministic: a verifier makes it itself and compares)
  python tools/gsc_keygen.py --srs-contribute SRS --out-dir D
      writes D/<name of SRS> and D/srs_contribution.record (544 bytes); the secrets come from the OS CSPRNG and are gone when the command
      returns
  python tools/gsc_keygen.py --verify-srs-contribution PREV NEXT RECORD
      prints ACCEPTED (exit status 0) or REFUSED (exit status 1; the library's line above it names the rule that failed).  PREV is not
      checked in full: verify a chain from --srs-initial's file, link by link
  python tools/gsc_keygen.py --verify-srs SRS
      prints ACCEPTED (exit status 0) or REFUSED (exit status 1; the library's line above it names the rule that failed)
  python tools/gsc_keygen.py --from-srs SRS R1CS PK VK
      checks the file, then writes a key pair with delta = gamma = 1.  SUCH A KEY IS FORGEABLE BY ANYONE: it becomes usable only after at
      least one --contribute, and a deployment verifies the file and every link of the chain
  python tools/gsc_keygen.py --verify-from-srs SRS R1CS PK VK
      is (PK, VK) what --from-srs makes of (SRS, R1CS)?  Byte for byte, but for the commitment key's sigma and g, which every run draws afresh
      and which must hold the Pedersen relation.  Prints ACCEPTED (exit status 0) or REFUSED (exit status 1): the start of a verified chain

Key ceremony, the Pedersen sigma: a key with a commitment (AES-128-V2, AES-256-V2) carries a second secret, sigma, which
whoever ran Setup held.  Every party re-randomises it like delta; sigma and delta links may interleave in one chain.

  python tools/gsc_keygen.py --contribute-sigma PK VK --out-dir D
      writes D/<name of PK>, D/<name of VK> and D/sigma_contribution.record (224 bytes); the secret comes from the OS CSPRNG and is gone when
      the command returns
  python tools/gsc_keygen.py --verify-sigma-contribution PREV_PK PREV_VK NEXT_PK NEXT_VK RECORD
      prints ACCEPTED (exit status 0) or REFUSED (exit status 1; the library's line above it names the rule that failed).  PREV's own
      Pedersen relation is not re-checked: verify a chain from a pair that passed --verify-from-srs or --verify-pedersen, link by link
  python tools/gsc_keygen.py --verify-pedersen PK VK
      prints ACCEPTED (exit status 0) or REFUSED (exit status 1): does the pair's commitment key hold the Pedersen relation?"""
import lzma
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _read(path):
    return lzma.open(path).read() if path.endswith(".xz") else open(path, "rb").read()


def contribute(g, args, sigma=False):
    if len(args) != 4 or args[2] != "--out-dir":
        raise SystemExit(__doc__)
    pk_path, vk_path, out = args[0], args[1], args[3]
    names = [os.path.basename(p)[:-3] if p.endswith(".xz") else os.path.basename(p) for p in (pk_path, vk_path)]
    if os.path.isdir(out) and any(os.path.abspath(os.path.join(out, n)) == os.path.abspath(p) for n, p in zip(names, (pk_path, vk_path))):
        raise SystemExit("--out-dir holds the input keys: choose another directory")
    pk, vk, record = (g.setup_contribute_sigma if sigma else g.setup_contribute)(_read(pk_path), _read(vk_path))
    os.makedirs(out, exist_ok=True)
    for name, b in zip(names + ["sigma_contribution.record" if sigma else "contribution.record"], (pk, vk, record)):
        open(os.path.join(out, name), "wb").write(b)
    print("pk %d bytes, vk %d bytes, record %d bytes -> %s" % (len(pk), len(vk), len(record), out))


def verify_contribution(g, args):
    if len(args) != 5:
        raise SystemExit(__doc__)
    ok = g.setup_verify_contribution(*[_read(p) for p in args])
    print("ACCEPTED" if ok else "REFUSED")
    raise SystemExit(0 if ok else 1)


def verdict(call, args, count):
    if len(args) != count:
        raise SystemExit(__doc__)
    ok = call(*[_read(p) for p in args])
    print("ACCEPTED" if ok else "REFUSED")
    raise SystemExit(0 if ok else 1)


def verify_srs(g, args):
    if len(args) != 1:
        raise SystemExit(__doc__)
    ok = g.srs_verify(_read(args[0]))
    print("ACCEPTED" if ok else "REFUSED")
    raise SystemExit(0 if ok else 1)


def srs_initial(g, args):
    if len(args) != 2:
        raise SystemExit(__doc__)
    srs = g.srs_initial(int(args[0]))
    open(args[1], "wb").write(srs)
    print("srs %d bytes -> %s" % (len(srs), args[1]))


def srs_contribute(g, args):
    if len(args) != 3 or args[1] != "--out-dir":
        raise SystemExit(__doc__)
    path, out = args[0], args[2]
    name = os.path.basename(path)[:-3] if path.endswith(".xz") else os.path.basename(path)
    if os.path.isdir(out) and os.path.abspath(os.path.join(out, name)) == os.path.abspath(path):
        raise SystemExit("--out-dir holds the input file: choose another directory")
    srs, record = g.srs_contribute(_read(path))
    os.makedirs(out, exist_ok=True)
    for n, b in ((name, srs), ("srs_contribution.record", record)):
        open(os.path.join(out, n), "wb").write(b)
    print("srs %d bytes, record %d bytes -> %s" % (len(srs), len(record), out))


def verify_srs_contribution(g, args):
    if len(args) != 3:
        raise SystemExit(__doc__)
    ok = g.srs_verify_contribution(*[_read(p) for p in args])
    print("ACCEPTED" if ok else "REFUSED")
    raise SystemExit(0 if ok else 1)


def from_srs(g, args):
    if len(args) != 4:
        raise SystemExit(__doc__)
    pk, vk = g.setup_from_srs(_read(args[1]), _read(args[0]))
    open(args[2], "wb").write(pk)
    open(args[3], "wb").write(vk)
    print("pk %d bytes, vk %d bytes; delta = 1: NOT usable before at least one --contribute" % (len(pk), len(vk)))


def main():
    import gsc_loader
    if len(sys.argv) > 1 and sys.argv[1] == "--verify-srs":
        return verify_srs(gsc_loader.load(), sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--srs-initial":
        return srs_initial(gsc_loader.load(), sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--srs-contribute":
        return srs_contribute(gsc_loader.load(), sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--verify-srs-contribution":
        return verify_srs_contribution(gsc_loader.load(), sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--from-srs":
        return from_srs(gsc_loader.load(), sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--contribute-sigma":
        return contribute(gsc_loader.load(), sys.argv[2:], sigma=True)
    if len(sys.argv) > 1 and sys.argv[1] == "--verify-sigma-contribution":
        return verdict(gsc_loader.load().setup_verify_sigma_contribution, sys.argv[2:], 5)
    if len(sys.argv) > 1 and sys.argv[1] == "--verify-pedersen":
        return verdict(gsc_loader.load().pedersen_verify, sys.argv[2:], 2)
    if len(sys.argv) > 1 and sys.argv[1] == "--verify-from-srs":
        g = gsc_loader.load()
        return verdict(lambda srs, r1cs, pk, vk: g.setup_verify_from_srs(r1cs, srs, pk, vk), sys.argv[2:], 4)
    if len(sys.argv) > 1 and sys.argv[1] == "--contribute":
        return contribute(gsc_loader.load(), sys.argv[2:])
    if len(sys.argv) > 1 and sys.argv[1] == "--verify-contribution":
        return verify_contribution(gsc_loader.load(), sys.argv[2:])
    if len(sys.argv) != 4:
        raise SystemExit(__doc__)
    g = gsc_loader.load()
    r1cs = _read(sys.argv[1])
    pk, vk = g.setup(r1cs)
    open(sys.argv[2], "wb").write(pk)
    open(sys.argv[3], "wb").write(vk)
    print("pk %d bytes -> %s, vk %d bytes -> %s" % (len(pk), sys.argv[2], len(vk), sys.argv[3]))


if __name__ == "__main__":
    main()
