"""Bit-level fingerprint of the GEMM entry points of one build of libaaclip_hip.so.

    AACLIP_LIB=ab/parent.so python tools/gemm_bits.py --out ab/bits_parent.json
    AACLIP_LIB=aa-clip_amd/aaclip/libaaclip_hip.so python tools/gemm_bits.py --out ab/bits_new.json
    python tools/gemm_bits.py --compare ab/bits_parent.json ab/bits_new.json

Runs a fixed, seeded table of launches at the tile edges and writes the SHA-256 of every output buffer
(C, the aux copy, the c_mx scales, the score partials). Two builds that compute the same thing give the
same file: there is no tolerance, a refactor that changes a bit has reordered something. Inputs come from
a CPU generator seeded by the case, outputs are pre-filled with a sentinel, so rows and columns a kernel
must not touch are part of the hash.

The table: aaclip_gemm under the tile families 0, 1, 2, 3, 8, 9, 11 for bf16 and fp16, M in {1, BM - 1,
BM + 1} x K of 1, 2, 3 K-steps x N in {BN, 2 BN} (N >= 128: the entry takes no less) with the epilogues
of tests/test_gemm_edges_gpu.py's ROTATION rotating over the cases; the fp32 kernel the same at its 64x64
tile; aaclip_gemm_scores on the same shapes with and without the LeakyReLU; aaclip_gemm_fp8; and
aaclip_gemm_fp8mx under variants 0 (8-phase) and 6 (256x256) with the eight epilogues of
tests/test_fp8_gpu.py::test_gemm_fp8mx_epilogues_at_tile_edges.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "aa-clip_amd"))

import torch  # noqa: E402

SENTINEL = -7.25  # exact in every dtype used here
TILES = {0: (256, 256), 1: (256, 256), 2: (256, 128), 3: (256, 256), 8: (320, 256), 9: (128, 128), 11: (64, 64)}
# (bias, activation, residual, aux, C dtype: "f32" or "h" = the operands' 16-bit type)
ROTATION = ((0, "", 0, 0, "f32"), (1, "", 0, 0, "h"), (1, "gelu", 0, 0, "h"), (1, "qgelu", 0, 0, "h"),
            (0, "leaky", 0, 0, "f32"), (1, "", 1, 0, "f32"), (1, "", 1, 1, "f32"), (0, "leaky", 1, 0, "h"),
            (1, "gelu", 1, 1, "f32"), (1, "", 0, 1, "h"), (0, "", 0, 0, "h"), (1, "", 0, 0, "f32"),
            (1, "gelu", 0, 0, "f32"), (1, "qgelu", 0, 0, "f32"), (0, "leaky", 0, 0, "h"), (1, "", 1, 0, "h"))
MX_EPILOGUES = ((1, "", 0, 0, "h"), (1, "", 1, 0, "f32"), (1, "", 1, 1, "f32"), (1, "gelu", 0, 0, "fp8"),
                (1, "qgelu", 0, 0, "fp8"), (0, "", 0, 0, "f32"), (0, "leaky", 0, 0, "f32"), (1, "", 1, 0, "h"))
FP8 = torch.float8_e4m3fn


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def cross(BM, ns, ks):
    for M in (1, BM - 1, BM + 1):
        for K in ks:
            for N in ns:
                yield M, N, K


def run(dev):
    from aaclip import _lib, ops
    out = {}
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731

    def rnd(seed, *shape, std=1.0):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(*shape, generator=g) * std

    def epilogue(seed, M, N, bias, act, resid, aux, cdt, hdt):
        kw = dict(bias=rnd(seed + 1, N, std=0.1).to(dev) if bias else None,
                  gelu={"gelu": True, "qgelu": "quick"}.get(act, False), leaky=act == "leaky",
                  residual=rnd(seed + 2, M, N).to(dev) if resid else None,
                  aux=torch.full((M, N), SENTINEL, dtype=hdt, device=dev) if aux else None)
        return torch.full((M, N), SENTINEL, dtype=cdt, device=dev), kw

    def variant(v):
        assert _lib.lib().aaclip_set_gemm_variant(v) == 0

    try:
        # ---- aaclip_gemm, 16-bit families, and aaclip_gemm_scores on the same operands
        for kind, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
            for fam, (BM, BN) in TILES.items():
                variant(fam)
                for i, (M, N, K) in enumerate(cross(BM, (max(BN, 128), 2 * max(BN, 128)), (64, 128, 192))):
                    bias, act, resid, aux, o = ROTATION[i % len(ROTATION)]
                    seed = 1000 * i + 7
                    a, w = rnd(seed, M, K).to(dt).to(dev), rnd(seed + 3, N, K, std=K ** -0.5).to(dt).to(dev)
                    c, kw = epilogue(seed, M, N, bias, act, resid, aux, torch.float32 if o == "f32" else dt, dt)
                    ops.gemm(a, w, c, **kw)
                    name = f"gemm {kind} fam{fam} M{M} N{N} K{K} {'bias+' * bias}{act}{'+resid' * resid}{'+aux' * aux}->{o}"
                    out[name] = {"C": sha(c)}
                    if aux:
                        out[name]["aux"] = sha(kw["aux"])
                    if N % 256 == 0:
                        tp = 64 if N == 256 else 128
                        T = rnd(seed + 5, tp, 2).to(dev)
                        part = torch.full((M, N // 8), SENTINEL, device=dev)
                        epi = _lib.EPI_LEAKY if (i // 2 + i) % 2 else 0  # both epilogues at both N
                        _lib.call("aaclip_gemm_scores", ops.dtag(a), M, N, K, ops._ptr(a), a.stride(0), ops._ptr(w),
                                  w.stride(0), epi, ops._ptr(T), tp, ops._ptr(part), part.stride(0), stream())
                        out[f"scores {kind} fam{fam} M{M} N{N} K{K} epi{epi}"] = {"part": sha(part)}
        variant(0)
        # ---- the fp32 kernel
        for i, (M, N, K) in enumerate(cross(64, (64, 128), (16, 32, 48))):
            bias, act, resid, aux, o = ROTATION[i % len(ROTATION)]
            seed = 1000 * i + 11
            a, w = rnd(seed, M, K).to(dev), rnd(seed + 3, N, K, std=K ** -0.5).to(dev)
            c, kw = epilogue(seed, M, N, bias, act, resid, aux, torch.float32 if o == "f32" else torch.bfloat16,
                             torch.bfloat16)
            ops.gemm(a, w, c, **kw)
            name = f"gemm f32 M{M} N{N} K{K} {'bias+' * bias}{act}{'+resid' * resid}{'+aux' * aux}->{o}"
            out[name] = {"C": sha(c)}
            if aux:
                out[name]["aux"] = sha(kw["aux"])

        def wq(seed, N, K):
            w = rnd(seed, N, K, std=K ** -0.5)
            s = w.abs().amax(dim=1).clamp_min(1e-30) / 448.0
            return (w / s[:, None]).to(FP8).to(dev), s.float().contiguous().to(dev)

        # ---- aaclip_gemm_fp8 (per-row scales): the 256x256 and the 256x128 kernel
        i = 0
        for M in (1, 255, 257):
            for K in (128, 256, 384):
                for N in (128, 256, 512):
                    bias, act, resid, aux, o = ROTATION[i % len(ROTATION)]
                    seed = 1000 * i + 13
                    i += 1
                    a = rnd(seed, M, K)
                    sa = (a.abs().amax(dim=1).clamp_min(1e-30) / 448.0).float()
                    a8 = (a / sa[:, None]).to(FP8).to(dev)
                    w8, sw = wq(seed + 3, N, K)
                    c, kw = epilogue(seed, M, N, bias, act, resid, aux,
                                     torch.float32 if o == "f32" else torch.bfloat16, torch.bfloat16)
                    ops.gemm_fp8(a8, sa.to(dev), w8, sw, c, **kw)
                    name = f"fp8 M{M} N{N} K{K} {'bias+' * bias}{act}{'+resid' * resid}{'+aux' * aux}->{o}"
                    out[name] = {"C": sha(c)}
                    if aux:
                        out[name]["aux"] = sha(kw["aux"])
        # ---- aaclip_gemm_fp8mx under the 8-phase kernel (0) and the 256x256 kernel (6)
        for v in (0, 6):
            variant(v)
            i = 0
            for M in (1, 255, 257):
                for N in (256, 512):
                    for K in (128, 256, 384):
                        bias, act, resid, aux, o = MX_EPILOGUES[i % len(MX_EPILOGUES)]
                        seed = 1000 * i + 17
                        i += 1
                        a8 = rnd(seed, M, K, std=8.0).to(FP8).to(dev)
                        ld = (M + 7) // 2 * 2  # padded, even
                        g = torch.Generator().manual_seed(seed + 4)
                        asc = torch.randint(120, 135, (K // 128, ld, 2), generator=g, dtype=torch.uint8).to(dev)
                        w8, sw = wq(seed + 3, N, K)
                        cdt = {"f32": torch.float32, "h": torch.bfloat16, "fp8": torch.uint8}[o]
                        rows = M + 3 if o == "fp8" else M  # fp8: padded, rows >= M must keep the sentinel
                        c = torch.full((rows, N), SENTINEL if o != "fp8" else 0x5A, dtype=cdt, device=dev)
                        _, kw = epilogue(seed, M, N, bias, act, resid, aux, torch.float32, torch.bfloat16)
                        csc = torch.full((N // 128, ld, 2), 0x5A, dtype=torch.uint8, device=dev) if o == "fp8" else None
                        ops.gemm_fp8mx(a8, asc, w8, sw, c.view(FP8) if o == "fp8" else c, out_sc=csc, **kw)
                        name = f"fp8mx v{v} M{M} N{N} K{K} {'bias+' * bias}{act}{'+resid' * resid}{'+aux' * aux}->{o}"
                        out[name] = {"C": sha(c)}
                        if aux:
                            out[name]["aux"] = sha(kw["aux"])
                        if csc is not None:
                            out[name]["c_mx"] = sha(csc)
    finally:
        _lib.lib().aaclip_set_gemm_variant(0)
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="JSON file to write the hashes to")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two hash files; with --out, write both columns")
    args = ap.parse_args()
    if args.compare:
        a, b = (json.load(open(p)) for p in args.compare)
        names = sorted(set(a["hashes"]) | set(b["hashes"]))
        bad = [n for n in names if a["hashes"].get(n) != b["hashes"].get(n)]
        if args.out:
            both = {n: {k: [a["hashes"].get(n, {}).get(k), b["hashes"].get(n, {}).get(k)]
                        for k in sorted(set(a["hashes"].get(n, {})) | set(b["hashes"].get(n, {})))} for n in names}
            json.dump({"libs": [a["lib"], b["lib"]], "launches": len(names), "differing": bad, "hashes": both},
                      open(args.out, "w"), indent=0, sort_keys=True)
        print(f"{len(names)} launches, {len(bad)} differ")
        for n in bad[:20]:
            print("  DIFFERS:", n)
        sys.exit(1 if bad else 0)
    hashes = run(torch.device("cuda:0"))
    from aaclip import _lib
    res = {"lib": os.path.relpath(_lib.LIB_PATH, ROOT), "hashes": hashes}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=0, sort_keys=True)
    print(f"{len(hashes)} launches hashed, digest of all: "
          f"{hashlib.sha256(json.dumps(hashes, sort_keys=True).encode()).hexdigest()[:16]}")


if __name__ == "__main__":
    main()
