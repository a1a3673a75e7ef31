"""The table of miseg_gemm launches (tests/test_gemm_plan_cpu.py; scripts/gemm_table.py launches the same rows on the card) and the sweep
over the seven question entry points.  A row is (id, params keywords, expected plan fields); the expected fields were worked out by hand from
the dispatcher's text as it stood before miseg_gemm_plan existed, not printed from the plan.  CPU only: the plan touches no device."""
import hashlib
import struct

A = 1 << 12      # an aligned stand-in address: the plan reads pointers for NULL and alignment only

NONE, RANK1, RANK1_STAT, SMALL, STREAM, NT_GENERIC, TN_STREAM, TN_GENERIC = range(8)      # MISEG_GEMM_* of include/miseg_hip.h
STORE, ACCUMULATE, ATOMIC = 0, 1, 2
BADARG, UNSUPPORTED = -1, -2
GELU = 2

QUESTIONS = ("miseg_gemm_fuses_stat", "miseg_gemm_fuses_anorm", "miseg_gemm_fuses_bstat", "miseg_gemm_fuses_scatter", "miseg_gemm_tn_fuses_colsum",
             "miseg_gemm_tn_splits", "miseg_gemm_workspace_bytes")


def params(L, M, N, K, tn=0, dt=1, odt=None, **f):
    """NT (tn=0): A [M][K], B [N][K], bf16 -> bf16, split_k 1.  TN (tn=1): A [K][M], B [K][N], -> fp32, split_k 0.  `an=n`: a folded norm of n
    styles; `scat=(d, h, w, cout)`; every other keyword is a field of miseg_gemm_params.  Optional row views get their natural row stride."""
    p = L.Gemm()
    p.A = p.B = p.C = A
    p.M, p.N, p.K, p.ta, p.tb, p.dtype = M, N, K, tn, tn, dt
    p.out_dtype = (0 if tn else dt) if odt is None else odt
    p.lda, p.ldb, p.ldc = (M, N, N) if tn else (K, K, N)
    p.split_k = 0 if tn else 1
    p.ldres = p.ldaux = p.ld_bs_x = N
    p.ld_an_out = K
    for k, v in f.items():
        if k == "an":
            p.an.stat, p.an.num_styles = A, v
        elif k == "an_styles":      # the styles alone: what miseg_gemm_fuses_anorm is asked with before the statistics exist
            p.an.num_styles = v
        elif k == "scat":
            p.scat_d, p.scat_h, p.scat_w, p.scat_cout = v
        else:
            setattr(p, k, v)
    return p


def answers(so, p):
    """the seven question entry points, in QUESTIONS order"""
    import ctypes as C
    return tuple(int(getattr(so, q)(C.byref(p))) for q in QUESTIONS)


def _r(id_, M, N, K, expect, **kw):
    return (id_, dict(M=M, N=N, K=K, **kw), expect)


BS = dict(stat=A, stat_mode=2, bs_x=A)      # a norm-backward-sums request
T0, T1, T2, T3, T4 = 110592, 13824, 1728, 216, 27      # tokens of the five Swin stages at 96^3 (48, 96, 192, 384, 768 channels)

ROWS = [
    # ---- the bench nets.  Swin stage 0 / 1: the streaming kernel (grid_x = min(cap, ceil(ceil(M / 32) / 4)), column groups to reach 300 workgroups)
    _r("s0-qkv", T0, 144, 48, dict(kernel=STREAM, k16=3, gelu=0, nch=12, stat=0, scat=0, anorm=1, grid_x=512, grid_y=1, cols_per_group=144, lds_bytes=17088), an=1, bias=A),
    _r("s0-proj", T0, 48, 48, dict(kernel=STREAM, k16=3, nch=6, stat=1, anorm=0, grid_x=512, grid_y=1, cols_per_group=48, lds_bytes=24960), res=A, stat=A, bias=A),
    _r("s0-fc1", T0, 192, 48, dict(kernel=STREAM, k16=3, gelu=1, nch=12, anorm=1, grid_x=512, grid_y=1, cols_per_group=192, lds_bytes=22656), an=1, act=GELU),
    _r("s0-fc2", T0, 48, 192, dict(kernel=STREAM, k16=12, nch=6, stat=1, grid_x=512, grid_y=1, cols_per_group=48, lds_bytes=24960), res=A, stat=A),
    _r("s1-qkv", T1, 288, 96, dict(kernel=STREAM, k16=6, nch=12, anorm=1, grid_x=108, grid_y=3, col_groups=3, cols_per_group=96, lds_bytes=21120), an=4),
    _r("s1-proj", T1, 96, 96, dict(kernel=STREAM, k16=6, nch=6, stat=1, grid_x=108, grid_y=3, cols_per_group=32, lds_bytes=16640), res=A, stat=A),
    _r("s1-fc1", T1, 384, 96, dict(kernel=STREAM, k16=6, gelu=1, nch=12, anorm=1, grid_x=108, grid_y=3, cols_per_group=128, lds_bytes=27904), an=1, act=GELU, an_out=A),
    _r("s1-fc2", T1, 96, 384, dict(kernel=STREAM, k16=24, nch=3, stat=0, grid_x=108, grid_y=3, cols_per_group=32, lds_bytes=25216, fuses_stat=0), res=A),
    # stage 2 .. 4: the small-M kernel; the tile is the candidate with the most workgroups in 140 .. 256, else the first with >= 140, else the last
    _r("s2-qkv", T2, 576, 192, dict(kernel=SMALL, mtw=2, ntw=4, anorm=1, stat=0, gelu=0, grid_x=486, row_tiles=54, col_groups=9, cols_per_group=64), an=1),
    _r("s2-proj", T2, 192, 192, dict(kernel=SMALL, mtw=2, ntw=4, stat=1, grid_x=162, row_tiles=54, col_groups=3), res=A, stat=A),
    _r("s2-fc1", T2, 768, 192, dict(kernel=SMALL, mtw=2, ntw=4, gelu=1, anorm=1, grid_x=648), an=1, act=GELU),
    _r("s2-fc2", T2, 192, 768, dict(kernel=SMALL, mtw=2, ntw=4, stat=1, grid_x=162), res=A, stat=A),
    _r("s3-qkv", T3, 1152, 384, dict(kernel=SMALL, mtw=2, ntw=2, anorm=1, grid_x=252, row_tiles=7, col_groups=36), an=1),
    _r("s3-proj", T3, 384, 384, dict(kernel=SMALL, mtw=2, ntw=1, stat=1, grid_x=168, row_tiles=7, col_groups=24), res=A, stat=A),
    _r("s3-fc1", T3, 1536, 384, dict(kernel=SMALL, mtw=2, ntw=4, gelu=1, anorm=1, grid_x=168), an=1, act=GELU),
    _r("s3-fc2", T3, 384, 1536, dict(kernel=SMALL, mtw=2, ntw=1, stat=1, grid_x=168), res=A, stat=A),
    _r("s4-qkv", T4, 2304, 768, dict(kernel=SMALL, mtw=2, ntw=1, anorm=0, grid_x=144, row_tiles=1, fuses_anorm=0), bias=A),      # K > 384: no folded norm
    _r("s4-proj", T4, 768, 768, dict(kernel=SMALL, mtw=1, ntw=1, stat=1, grid_x=96, row_tiles=2, col_groups=48, cols_per_group=16), res=A, stat=A),
    _r("s4-fc1", T4, 3072, 768, dict(kernel=SMALL, mtw=2, ntw=1, gelu=1, grid_x=192), act=GELU, aux=A, epi_mode=1),
    _r("s4-fc2", T4, 768, 3072, dict(kernel=SMALL, mtw=1, ntw=1, grid_x=96), res=A),
    # patch merging: Linear(8C -> 2C) on an eighth of the tokens
    _r("merge-0", T1, 96, 384, dict(kernel=STREAM, k16=24, nch=3, grid_x=108, grid_y=3, lds_bytes=25216)),
    _r("merge-1", T2, 192, 768, dict(kernel=SMALL, mtw=2, ntw=4, grid_x=162)),
    _r("merge-2", T3, 384, 1536, dict(kernel=SMALL, mtw=2, ntw=1, grid_x=168)),
    _r("merge-3", T4, 768, 3072, dict(kernel=SMALL, mtw=1, ntw=1, grid_x=96)),
    # 1x1x1 shortcut convolutions of the residual blocks (statistics of the output for the norm behind them) and the rank-1 stem shortcut
    _r("sc-96^3-96-48", 884736, 48, 96, dict(kernel=STREAM, k16=6, nch=6, stat=1, grid_x=512, grid_y=1, lds_bytes=24960), stat=A),
    _r("sc-48^3-192-96", T0, 96, 192, dict(kernel=STREAM, k16=12, nch=6, stat=1, grid_x=512, grid_y=1, cols_per_group=96, lds_bytes=49920), stat=A),
    _r("sc-24^3-384-192", T1, 192, 384, dict(kernel=NT_GENERIC, nt=4, grid_x=108, grid_y=3, grid_z=1, splits=1, k_per_split=384, out_mode=STORE, zero_fill=0, fuses_stat=0, al_a=1, al_b=1)),
    _r("stem-rank1-stat", 884736, 48, 1, dict(kernel=RANK1_STAT, grid_x=2048, grid_y=1, grid_z=1, fuses_stat=1), stat=A),
    _r("stem-rank1", 884736, 48, 1, dict(kernel=RANK1, grid_x=8192, fuses_stat=1)),
    _r("stem-rank1-f32", 4096, 32, 1, dict(kernel=RANK1_STAT, grid_x=128), dt=0, stat=A),      # 256 / (32 / 4) = 32 rows per workgroup
    # ConvTranspose3d(k2, s2) as a GEMM: the scattered store where the streaming kernel runs, a plain product below 4096 voxels
    _r("up-24^3-96-48", T1, 384, 96, dict(kernel=STREAM, k16=6, nch=12, scat=1, stat=0, grid_x=108, grid_y=1, col_groups=1, cols_per_group=384, lds_bytes=81408, fuses_scatter=1), scat=(24, 24, 24, 48)),
    _r("up-48^3-48-48", T0, 384, 48, dict(kernel=STREAM, k16=3, nch=12, scat=1, grid_x=512, grid_y=1, lds_bytes=44544), scat=(48, 48, 48, 48)),
    _r("up-12^3-192", T2, 768, 192, dict(kernel=SMALL, mtw=2, ntw=4, grid_x=648, fuses_scatter=0)),
    _r("up-6^3-384", T3, 1536, 384, dict(kernel=SMALL, mtw=2, ntw=4, grid_x=168)),
    _r("up-3^3-768", T4, 3072, 768, dict(kernel=SMALL, mtw=2, ntw=1, grid_x=192)),
    # C-UNETR's ViT: 216 tokens of 768 channels
    _r("vit-qkv", 216, 2304, 768, dict(kernel=SMALL, mtw=2, ntw=4, grid_x=252)),
    _r("vit-proj", 216, 768, 768, dict(kernel=SMALL, mtw=2, ntw=2, grid_x=168), res=A, bias=A),
    _r("vit-fc1", 216, 3072, 768, dict(kernel=SMALL, mtw=4, ntw=3, gelu=1, grid_x=256, row_tiles=4, col_groups=64, cols_per_group=48), act=GELU, bias=A),
    _r("vit-fc2", 216, 768, 3072, dict(kernel=SMALL, mtw=2, ntw=2, grid_x=168), res=A),
    # weight gradients dW[M][N] = A[K][M]^T B[K][N]: tall ones stream (384 workgroups wanted, >= 256 rows a split), short ones take the generic kernel
    _r("tn-s0-qkv", 144, 48, T0, dict(kernel=TN_STREAM, wm=4, wn=1, grid_x=1, grid_y=1, grid_z=346, splits=346, k_per_split=320, lds_bytes=65536, workspace_bytes=9566208,
                                       out_mode=STORE, reduce_groups=22, reduce_blocks=7, zero_fill=1, tn_fuses_colsum=1), tn=1, workspace=A),
    _r("tn-s0-fc2", 48, 192, T0, dict(kernel=TN_STREAM, wm=1, wn=4, grid_x=1, grid_y=1, splits=346, lds_bytes=65536, out_mode=ACCUMULATE, zero_fill=0, reduce_groups=22), tn=1, workspace=A, accumulate=1),
    _r("tn-s1-fc1", 384, 96, T1, dict(kernel=TN_STREAM, wm=2, wn=2, grid_x=4, grid_y=1, grid_z=54, splits=54, k_per_split=256, lds_bytes=53248, workspace_bytes=7962624, reduce_groups=4,
                                       reduce_blocks=36), tn=1, workspace=A, tn_colsum=A),
    _r("tn-s1-fc1-deferred", 384, 96, T1, dict(kernel=TN_STREAM, splits=54, reduce_groups=0, reduce_blocks=0, zero_fill=0), tn=1, workspace=A, defer_reduce=1),
    _r("tn-s3-proj", 384, 384, T3, dict(kernel=TN_GENERIC, grid_x=6, grid_y=6, grid_z=1, splits=1, k_per_split=256, out_mode=ACCUMULATE, zero_fill=0, tn_fuses_colsum=0, workspace_bytes=0), tn=1, accumulate=1),
    _r("tn-s2-proj", 192, 192, T2, dict(kernel=TN_GENERIC, grid_x=3, grid_y=3, grid_z=4, splits=4, k_per_split=512, out_mode=ATOMIC, zero_fill=1), tn=1),
    # ---- the edges of each predicate
    _r("m15-small", 15, 64, 64, dict(kernel=SMALL, mtw=1, ntw=1, grid_x=4, fuses_stat=0, fuses_anorm=0, fuses_bstat=0), an_styles=1, bs_x=A),
    _r("m15-stat-refused", 15, 64, 64, dict(rc=UNSUPPORTED, kernel=NONE, fuses_stat=0), stat=A),
    _r("m16-small-stat", 16, 64, 64, dict(kernel=SMALL, mtw=1, ntw=1, stat=1, grid_x=4, row_tiles=1, fuses_stat=1), stat=A),
    _r("m2048-small", 2048, 384, 64, dict(kernel=SMALL, mtw=4, ntw=3, grid_x=256, row_tiles=32, col_groups=8)),
    _r("m2049-generic", 2049, 384, 64, dict(kernel=NT_GENERIC, nt=4, grid_x=17, grid_y=6, k_per_split=64, fuses_stat=0)),
    _r("m4095-generic", 4095, 48, 48, dict(kernel=NT_GENERIC, nt=3, grid_x=32, grid_y=1, fuses_stat=0)),
    _r("m4096-stream", 4096, 48, 48, dict(kernel=STREAM, k16=3, nch=12, grid_x=32, grid_y=3, cols_per_group=16, lds_bytes=1856, fuses_stat=1)),
    _r("k32-odd-small", 2048, 64, 48, dict(kernel=NT_GENERIC, nt=4)),      # K % 32 != 0 and M < 4096
    _r("k144", T0, 48, 144, dict(kernel=STREAM, k16=9, nch=12, gelu=1, fuses_stat=0, fuses_anorm=0, fuses_scatter=0), act=GELU),
    _r("k192", T0, 48, 192, dict(kernel=STREAM, k16=12, nch=12, fuses_stat=1, fuses_anorm=0)),
    _r("k288", T0, 48, 288, dict(kernel=STREAM, k16=18, nch=6, fuses_stat=0)),
    _r("k384", T0, 48, 384, dict(kernel=STREAM, k16=24, nch=3, gelu=1, fuses_bstat=0), act=GELU, bs_x=A),
    _r("k240-generic", T0, 48, 240, dict(kernel=NT_GENERIC, nt=3, grid_x=864, k_per_split=256)),
    _r("stat-n96", T0, 96, 48, dict(kernel=STREAM, stat=1, nch=6, k16=3, fuses_stat=1), stat=A),
    _r("stat-n112-refused", T0, 112, 48, dict(rc=UNSUPPORTED, kernel=NONE, fuses_stat=0), stat=A),
    _r("stat-k144-refused", T0, 48, 144, dict(rc=UNSUPPORTED, fuses_stat=0), stat=A),
    _r("anorm-k192-refused", T0, 48, 192, dict(rc=UNSUPPORTED, fuses_anorm=0), an=1),
    _r("anorm-styles0-refused", T0, 48, 48, dict(rc=UNSUPPORTED, fuses_anorm=0), an=0),
    _r("anorm-styles5-refused", T0, 48, 48, dict(rc=UNSUPPORTED, fuses_anorm=0), an=5),
    _r("anorm-an_out-off8-refused", T0, 48, 48, dict(rc=UNSUPPORTED, fuses_anorm=0), an=1, an_out=A + 8),
    _r("anorm-small-k416-refused", 216, 64, 416, dict(rc=UNSUPPORTED, fuses_anorm=0), an=1),
    _r("scat-k144-refused", T0, 384, 144, dict(rc=UNSUPPORTED, fuses_scatter=0), scat=(48, 48, 48, 48)),
    _r("scat-rows-refused", T0, 384, 48, dict(rc=UNSUPPORTED, fuses_scatter=0), scat=(48, 48, 47, 48)),
    _r("bstat-k48", T0, 48, 48, dict(kernel=STREAM, k16=3, nch=6, stat=2, grid_x=512, grid_y=1, cols_per_group=48, lds_bytes=24960, fuses_bstat=1), **BS),
    _r("bstat-k144", T0, 48, 144, dict(kernel=STREAM, k16=9, nch=6, stat=2, fuses_bstat=1), **BS),
    _r("bstat-k288-two-chunks", T0, 96, 288, dict(kernel=STREAM, k16=18, nch=3, stat=2, grid_x=512, grid_y=2, col_groups=2, cols_per_group=48, lds_bytes=28992), **BS),
    _r("bstat-k384-refused", T0, 96, 384, dict(rc=UNSUPPORTED, fuses_bstat=0), **BS),
    _r("bstat-n144-refused", T0, 144, 48, dict(rc=UNSUPPORTED, fuses_bstat=0), **BS),
    _r("bstat-bs_x-off4-refused", T0, 48, 48, dict(rc=UNSUPPORTED, fuses_bstat=0), stat=A, stat_mode=2, bs_x=A + 4),
    _r("bstat-small-n384", T3, 384, 384, dict(kernel=SMALL, mtw=2, ntw=1, stat=2, grid_x=168, fuses_bstat=1), **BS),
    _r("bstat-small-n400-refused", T3, 400, 384, dict(rc=UNSUPPORTED, fuses_bstat=0), **BS),
    _r("stat_mode1-refused", T0, 48, 48, dict(rc=BADARG), stat=A, stat_mode=1),
    _r("lds-80k-below", T0, 384, 96, dict(kernel=STREAM, grid_x=512, grid_y=1, cols_per_group=384, lds_bytes=81408)),
    _r("lds-80k-above", T0, 400, 96, dict(kernel=STREAM, grid_x=256, grid_y=5, col_groups=5, cols_per_group=80, lds_bytes=16960)),      # 84800 bytes of weight: 256 workgroups
    _r("lds-96k-below", T0, 448, 96, dict(kernel=STREAM, grid_x=256, grid_y=2, cols_per_group=224)),
    _r("lds-96k-above", T0, 464, 96, dict(kernel=NT_GENERIC, nt=4, grid_x=864, grid_y=8)),      # 98368 bytes
    # the small kernel's tile: (4, 3) and rule one are in the bench rows above ((2, 4) s2-proj, (2, 2) s3-qkv, (2, 1) s3-proj); the rest
    _r("tile-2x4-fallback", T2, 576, 64, dict(kernel=SMALL, mtw=2, ntw=4, grid_x=486)),
    _r("tile-2x2-fallback", 2048, 160, 64, dict(kernel=SMALL, mtw=2, ntw=2, grid_x=320)),
    _r("tile-2x1-fallback", 2048, 80, 64, dict(kernel=SMALL, mtw=2, ntw=1, grid_x=320)),
    _r("tile-1x2-rule1", 16, 4608, 64, dict(kernel=SMALL, mtw=1, ntw=2, grid_x=144, row_tiles=1, col_groups=144, cols_per_group=32)),
    _r("tile-1x2-fallback", 16, 16384, 64, dict(kernel=SMALL, mtw=1, ntw=2, grid_x=512)),
    # (2, 1) would be 11 x 24 = 264 workgroups, over the 256 of rule one; (1, 2) is 21 x 12 = 252 - with the norm-backward sums, N <= 384
    _r("tile-1x2-rule1-m330-bstat", 330, 384, 64, dict(kernel=SMALL, mtw=1, ntw=2, stat=2, grid_x=252, row_tiles=21, col_groups=12, cols_per_group=32, fuses_bstat=1), **BS),
    _r("tile-1x2-rule1-m1350", 1350, 96, 64, dict(kernel=SMALL, mtw=1, ntw=2, grid_x=255, row_tiles=85, col_groups=3)),
    _r("tile-1x1-rule1", 16, 2320, 64, dict(kernel=SMALL, mtw=1, ntw=1, grid_x=145)),
    _r("tile-1x1-last", T4, 384, 64, dict(kernel=SMALL, mtw=1, ntw=1, grid_x=48)),
    _r("tile-4x3-needs-m33", 32, 12288, 64, dict(kernel=SMALL, mtw=2, ntw=4, grid_x=192)),      # (4, 3) would be 256 workgroups, but needs M > 32
    # misaligned operands, one field at a time: off the two bf16 kernels, the generic one reads A / B by elements where it must
    _r("a-off2", T0, 48, 48, dict(kernel=NT_GENERIC, nt=3, al_a=0, al_b=1, grid_x=864, grid_y=1), A=A + 2),
    _r("b-off8", T0, 48, 48, dict(kernel=NT_GENERIC, al_a=1, al_b=0), B=A + 8),
    _r("c-off4", T0, 48, 48, dict(kernel=NT_GENERIC, al_a=1, al_b=1), C=A + 4),
    _r("c-off8", T0, 48, 48, dict(kernel=STREAM), C=A + 8),
    _r("res-off4", T0, 48, 48, dict(kernel=NT_GENERIC), res=A + 4),
    _r("aux-off4", T0, 48, 48, dict(kernel=NT_GENERIC), aux=A + 4, epi_mode=1),
    _r("aux-off4-unused", T0, 48, 48, dict(kernel=STREAM), aux=A + 4),
    _r("lda-odd", T0, 48, 48, dict(kernel=NT_GENERIC, al_a=0), lda=49),
    _r("ldb-52", T0, 48, 48, dict(kernel=NT_GENERIC, al_b=0), ldb=52),
    _r("ldc-odd", T0, 48, 48, dict(kernel=NT_GENERIC), ldc=49),
    _r("ldres-50", T0, 48, 48, dict(kernel=NT_GENERIC), res=A, ldres=50),
    _r("small-a-off2", T3, 384, 384, dict(kernel=NT_GENERIC, nt=4, al_a=0, grid_x=2, grid_y=6), A=A + 2),
    # split_k and accumulate
    _r("nt-f32-split0", 256, 64, 512, dict(kernel=NT_GENERIC, nt=4, grid_x=2, grid_y=1, grid_z=1, splits=1, k_per_split=512, out_mode=STORE, zero_fill=0), dt=0, split_k=0),
    _r("nt-f32-split1-acc", 256, 64, 512, dict(kernel=NT_GENERIC, splits=1, out_mode=ACCUMULATE, zero_fill=0), dt=0, accumulate=1),
    _r("nt-f32-split4", 256, 64, 512, dict(kernel=NT_GENERIC, grid_z=4, splits=4, k_per_split=128, out_mode=ATOMIC, zero_fill=1), dt=0, split_k=4),
    _r("nt-f32-split4-acc", 256, 64, 512, dict(kernel=NT_GENERIC, splits=4, out_mode=ATOMIC, zero_fill=0), dt=0, split_k=4, accumulate=1),
    _r("nt-bf16-f32-split4", 256, 40, 512, dict(kernel=NT_GENERIC, nt=3, grid_y=1, splits=4, k_per_split=128, out_mode=ATOMIC, zero_fill=1), odt=0, split_k=4),
    _r("nt-f32-split4-one-stage", 64, 64, 32, dict(kernel=NT_GENERIC, splits=1, k_per_split=32, out_mode=ATOMIC, zero_fill=0), dt=0, split_k=4),
    _r("nt-bf16-split4-refused", 256, 64, 512, dict(rc=BADARG), split_k=4),
    _r("nt-bf16-acc-refused", 256, 64, 512, dict(rc=BADARG), accumulate=1),
    _r("nt-split4-gelu-refused", 256, 64, 512, dict(rc=BADARG), dt=0, split_k=4, act=GELU),
    _r("nt-split4-res-refused", 256, 64, 512, dict(rc=BADARG), dt=0, split_k=4, res=A),
    _r("rank1-f32-split4", 4096, 32, 1, dict(kernel=RANK1, grid_x=128, fuses_stat=0), dt=0, split_k=4),
    _r("rank1-n136", 4096, 136, 1, dict(kernel=RANK1, grid_x=272, fuses_stat=0)),
    _r("tn-split1", 192, 192, T2, dict(kernel=TN_GENERIC, splits=1, k_per_split=1792, out_mode=STORE, zero_fill=0, grid_z=1), tn=1, split_k=1),
    _r("tn-split4", 192, 192, T2, dict(kernel=TN_GENERIC, splits=4, k_per_split=512, out_mode=ATOMIC, zero_fill=1), tn=1, split_k=4),
    _r("tn-split4-acc", 192, 192, T2, dict(kernel=TN_GENERIC, splits=4, out_mode=ATOMIC, zero_fill=0), tn=1, split_k=4, accumulate=1),
    _r("tn-f32", 96, 96, T2, dict(kernel=TN_GENERIC, grid_x=2, grid_y=2, splits=4, k_per_split=448), tn=1, dt=0),
    _r("tn-tall-split1-not-streamed", 144, 48, T0, dict(kernel=TN_GENERIC, splits=1, tn_fuses_colsum=0, workspace_bytes=0), tn=1, split_k=1),
    _r("tn-stream-k2047", 144, 48, 2047, dict(kernel=TN_GENERIC, tn_fuses_colsum=0), tn=1),
    _r("tn-stream-m40", 40, 48, T0, dict(kernel=TN_GENERIC, tn_fuses_colsum=0), tn=1),
    _r("tn-stream-a-off8", 144, 48, T0, dict(kernel=TN_GENERIC, tn_fuses_colsum=0, al_a=0), tn=1, A=A + 8),
    _r("tn-stream-one-split", 1920, 1920, 2048, dict(kernel=TN_STREAM, wm=2, wn=2, grid_x=20, grid_y=20, grid_z=1, splits=1, k_per_split=2048, workspace_bytes=0, reduce_groups=0, zero_fill=0), tn=1),
    _r("tn-stream-one-group", 480, 480, 4096, dict(kernel=TN_STREAM, grid_x=5, grid_y=5, splits=16, k_per_split=256, reduce_groups=1, reduce_blocks=225, zero_fill=0, workspace_bytes=14745600), tn=1, workspace=A),
    _r("tn-colsum-not-streamed-refused", 192, 192, T2, dict(rc=UNSUPPORTED, tn_fuses_colsum=0), tn=1, tn_colsum=A),
    _r("tn-bias-refused", 144, 48, T0, dict(rc=UNSUPPORTED, tn_fuses_colsum=1, workspace_bytes=9566208, splits=346), tn=1, bias=A),
    _r("ta0-tb1-refused", 64, 64, 64, dict(rc=UNSUPPORTED), tb=1),
    _r("act1-refused", 64, 64, 64, dict(rc=UNSUPPORTED), act=1),
    _r("dtype-f32-bf16-refused", 64, 64, 64, dict(rc=BADARG), dt=0, odt=1),
    _r("epi-mode-no-aux-refused", 64, 64, 64, dict(rc=BADARG), epi_mode=2),
    _r("null-a-refused", 64, 64, 64, dict(rc=BADARG), A=None),
    _r("m0-refused", 0, 64, 64, dict(rc=BADARG)),
]
# every instantiation a plan may name.  gemm_nt_small_kernel<MTW, NTW, GELU, STAT, ANORM>: six tiles x (plain, GELU, norm, norm + GELU, statistics,
# norm-backward sums)
SMALL_TILES = [(4, 3), (2, 4), (2, 2), (2, 1), (1, 2), (1, 1)]
SMALL_FORMS = {(m, n, g, s, a) for m, n in SMALL_TILES for g, s, a in [(0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 0, 1), (0, 1, 0), (0, 2, 0)]}
# gemm_nt_stream_kernel<K16, GELU, NCH, STAT, SCAT, ANORM>
STREAM_FORMS = {(k, g, 12 if k <= 12 else 6 if k == 18 else 3, 0, 0, 0) for k in (3, 6, 9, 12, 18, 24) for g in (0, 1)} | {
    (k, g, 12, 0, 0, 1) for k in (3, 6) for g in (0, 1)} | {(k, 0, 6, 1, 0, 0) for k in (3, 6, 12)} | {
    (3, 0, 6, 2, 0, 0), (6, 0, 6, 2, 0, 0), (9, 0, 6, 2, 0, 0), (12, 0, 6, 2, 0, 0), (18, 0, 3, 2, 0, 0), (3, 0, 12, 0, 1, 0), (6, 0, 12, 0, 1, 0)}

# a shape per tile of the small kernel (N <= 384: the norm-backward sums) and the requests laid over it
SMALL_TILE_SHAPES = {(4, 3): (2048, 384), (2, 4): (T2, 192), (2, 2): (2048, 96), (2, 1): (T3, 384), (1, 2): (330, 384), (1, 1): (T4, 384)}
REQUESTS = {(0, 0, 0): {}, (1, 0, 0): dict(act=GELU), (0, 0, 1): dict(an=1), (1, 0, 1): dict(an=1, act=GELU), (0, 1, 0): dict(stat=A), (0, 2, 0): BS}


def launcher_forms():
    """(small, stream): the instantiation lists of csrc/gemm.hip's launchers (NT_SMALL_FORMS, NT_STREAM_FORMS), read from the source"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mi-seg_amd", "csrc", "gemm.hip")).read()
    val = {"true": 1, "false": 0}

    def body(name):      # the macro's replacement text: its line and the continuation lines behind it
        lines = src[src.index("#define %s(" % name):].split("\n")
        n = next(i for i, ln in enumerate(lines) if not ln.rstrip().endswith("\\"))
        return " ".join(ln.rstrip().rstrip("\\") for ln in lines[:n + 1]).split(")", 1)[1]

    def args(text):
        return tuple(int(val.get(t.strip(), t.strip())) for t in text.split(","))

    epilogues = [args(m) for m in re.findall(r"X\(m_, n_,([^)]*)\)", body("NT_SMALL_EPILOGUES"))]
    tiles = [args(m) for m in re.findall(r"NT_SMALL_EPILOGUES\(X,([^)]*)\)", body("NT_SMALL_FORMS"))]
    small = [t + e for t in tiles for e in epilogues]
    stream = [args(m) for m in re.findall(r"X\(([^)]*)\)", body("NT_STREAM_FORMS"))]
    return small, stream


def form_rows():
    """(params keywords, the instantiation the row is there for): every small and every stream form, each from a shape and a request"""
    out = []
    for (m, n, g, s, a) in sorted(SMALL_FORMS):
        M, N = SMALL_TILE_SHAPES[(m, n)]
        out.append((dict(M=M, N=N, K=64, **REQUESTS[(g, s, a)]), ("small", m, n, g, s, a)))
    for (k, g, nch, s, sc, a) in sorted(STREAM_FORMS):
        kw = dict(REQUESTS[(g, s, a)])
        if sc:
            kw["scat"] = (48, 48, 48, 48)
        out.append((dict(M=T0, N=384 if sc else 48, K=16 * k, **kw), ("stream", k, g, nch, s, sc, a)))
    return out


# ---- the sweep over the question entry points
M_VALUES = [1, 15, 16, 17, 27, 32, 33, 48, 216, 1728, 2047, 2048, 2049, 4095, 4096, 4097, 13824, 110592]
N_VALUES = [1, 4, 8, 16, 32, 40, 48, 64, 96, 112, 128, 136, 144, 192, 288, 384, 400, 448, 464, 768, 3072]
K_VALUES = [1, 16, 32, 48, 64, 96, 144, 192, 240, 288, 384, 416, 768, 2047, 2048, 2049, 4096, 13824, 110592]
OFFSETS = [0, 2, 4, 8]
SLACK = [0, 1, 4, 8]
# (field, values) with the plain value first: a draw takes the plain value three times out of four
OPTIONS = [
    ("tn", [0, 1]), ("dtypes", [(1, 1), (0, 0), (1, 0)]), ("a_off", OFFSETS), ("b_off", OFFSETS), ("c_off", OFFSETS), ("lda_slack", SLACK), ("ldb_slack", SLACK),
    ("ldc_slack", SLACK), ("split_k", [1, 0, 4, 2]), ("accumulate", [0, 1]), ("act", [0, GELU, 1]), ("res", [None, 0, 2, 4, 8]), ("ldres_slack", SLACK),
    ("aux", [None, 0, 4, 8]), ("ldaux_slack", SLACK), ("epi_mode", [0, 1, 2]), ("stat", [None, A]), ("stat_mode", [0, 2, 1]), ("an_stat", [None, A]),
    ("an_styles", [1, 0, 4, 5]), ("an_out", [None, 0, 8, 4]), ("ld_an_out_slack", SLACK), ("bs_x", [None, 0, 4, 8]), ("ld_bs_x_slack", SLACK),
    ("scat_cout", [0, "N/8", 4, -4]), ("scat_grid", [(1, 1, 1), (2, 2, 2), (48, 48, 48), (0, 1, 1), (3, 3, 3), (16, 16, 16)]), ("bias", [None, A]),
    ("workspace", [None, A]), ("defer_reduce", [0, 1]), ("tn_colsum", [None, A]), ("ta_tb_mixed", [0, 1]),
]


def _build(L, M, N, K, o):
    def view(off):
        return None if off is None else A + off
    tn = o["tn"]
    p = params(L, M, N, K, tn=tn, dt=o["dtypes"][0], odt=o["dtypes"][1])
    p.A, p.B, p.C = A + o["a_off"], A + o["b_off"], A + o["c_off"]
    p.lda += o["lda_slack"]; p.ldb += o["ldb_slack"]; p.ldc += o["ldc_slack"]
    if o["ta_tb_mixed"]:
        p.tb = 1 - p.tb
    p.split_k, p.accumulate, p.act, p.epi_mode, p.stat, p.stat_mode = o["split_k"], o["accumulate"], o["act"], o["epi_mode"], o["stat"], o["stat_mode"]
    p.res, p.ldres, p.aux, p.ldaux = view(o["res"]), N + o["ldres_slack"], view(o["aux"]), N + o["ldaux_slack"]
    p.an.stat, p.an.num_styles, p.an_out, p.ld_an_out = o["an_stat"], o["an_styles"], view(o["an_out"]), K + o["ld_an_out_slack"]
    p.bs_x, p.ld_bs_x = view(o["bs_x"]), N + o["ld_bs_x_slack"]
    p.scat_cout = N // 8 if o["scat_cout"] == "N/8" else o["scat_cout"]
    p.scat_d, p.scat_h, p.scat_w = o["scat_grid"]
    p.bias, p.workspace, p.defer_reduce, p.tn_colsum = o["bias"], o["workspace"], o["defer_reduce"], o["tn_colsum"]
    return p


def sweep(so, L, count, seed, each=None):
    """sha256 over the seven answers of `count` drawn parameter sets and of every single-field variation of every launched table row's shape;
    returns (hex digest, parameter sets asked, how many of them each question answered with non-zero).  each(p): called with every set."""
    state = [seed & (2 ** 64 - 1)]

    def draw(n):      # a 64-bit LCG of our own (Knuth's MMIX constants): the same draws under every Python
        state[0] = (state[0] * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (state[0] >> 33) % n

    h = hashlib.sha256()
    asked, yes = 0, [0] * len(QUESTIONS)

    def ask(p):
        nonlocal asked
        a = answers(so, p)
        h.update(struct.pack("<7q", *a))
        asked += 1
        if each is not None:
            each(p)
        for i, v in enumerate(a):
            yes[i] += bool(v)

    plain = {f: vs[0] for f, vs in OPTIONS}
    for _ in range(count):
        o = {f: (vs[0] if draw(4) else vs[draw(len(vs))]) for f, vs in OPTIONS}
        o["tn"] = int(draw(3) == 0)
        if o["tn"] and draw(4):      # a weight gradient's plain form: bf16 -> fp32, the library's own split
            o["dtypes"], o["split_k"] = (1, 0), 0
        ask(_build(L, M_VALUES[draw(len(M_VALUES))], N_VALUES[draw(len(N_VALUES))], K_VALUES[draw(len(K_VALUES))], o))
    for _, kw, expect in ROWS:
        if expect.get("rc", 0) != 0 or kw["M"] <= 0:
            continue
        base = dict(plain, tn=kw.get("tn", 0), dtypes=(kw.get("dt", 1), kw.get("odt", 0 if kw.get("tn", 0) else kw.get("dt", 1))))
        if not kw.get("tn", 0):
            base["split_k"] = 1
        else:
            base["split_k"] = 0
        for f, vs in OPTIONS:
            for v in vs:
                ask(_build(L, kw["M"], kw["N"], kw["K"], dict(base, **{f: v})))
        for M in M_VALUES:
            ask(_build(L, M, kw["N"], kw["K"], base))
        for N in N_VALUES:
            ask(_build(L, kw["M"], N, kw["K"], base))
        for K in K_VALUES:
            ask(_build(L, kw["M"], kw["N"], K, base))
    return h.hexdigest(), asked, dict(zip(QUESTIONS, yes))
