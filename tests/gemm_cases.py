"""The table of miseg_gemm launches (tests/test_gemm_plan_cpu.py; scripts/gemm_table.py launches the same rows on the card) and the sweep
over the seven question entry points.  A row is (id, params keywords, expected plan fields); the expected fields were worked out by hand from
the dispatcher's text as it stood before miseg_gemm_plan existed, not printed from the plan.  FORM_ROWS (further down) are the card-sized
rows of every form that tests/test_hip_gemm_forms.py launches and judges.  CPU only: the plan touches no device."""
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
    _r("nt-f32-split4-one-stage", 64, 64, 32, dict(kernel=NT_GENERIC, splits=1, k_per_split=32, out_mode=STORE, zero_fill=0), dt=0, split_k=4),
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


# ================================================================================================ the rows launched on the card
# FORM_ROWS: card-sized launches of every form (tests/test_hip_gemm_forms.py launches each; tests/test_gemm_plan_cpu.py pins the plans here).
# A row is (id, keywords, expected plan fields); the id spells the form, the expected fields were worked out by hand from gemm_plan's text.
# Keywords: M, N, K, tn, dt, odt as in params(); bias / res / stat / bstat / an_out / colsum / defer / ints = 1; act; epi = epi_mode (aux is
# implied); an = number of styles of a folded norm; scat = (d, h, w, cout) with M = B d h w; split_k; accumulate; lay = {operand: layout of
# tests/layouts.py} for the row views A, B, C, res, aux, bs_x, an_out ("left": the left half of rows twice as wide, the scattered store's C).
ES = {0: 4, 1: 2}      # bytes per element of MISEG_F32 / MISEG_BF16


def layout(c, es, lay):
    """(element offset of the view's first column, row stride) of a row view of c columns: what tests/layouts.py::Slot builds"""
    n = 16 // es
    cp = -(-c // n) * n
    return {"contig": (0, c), "slice": (n, cp + 3 * n), "off8": (n // 2, cp + 2 * n), "ldodd": (0, cp + n + 1), "off4": (n // 4, cp + 2 * n),
            "off2": (n // 8, cp + 2 * n), "left": (0, 2 * c)}[lay]


def dtypes(kw):
    tn, dt = kw.get("tn", 0), kw.get("dt", 1)
    return dt, kw.get("odt", 0 if tn else dt)


def operand_cols(kw):
    """name -> (columns, bytes per element) of every row view the row's launch passes"""
    dt, odt = dtypes(kw)
    M, N, K = kw["M"], kw["N"], kw["K"]
    if kw.get("tn", 0):
        return dict(A=(M, ES[dt]), B=(N, ES[dt]), C=(N, ES[odt]))
    d = dict(A=(K, ES[dt]), B=(K, ES[dt]), C=(kw["scat"][3] if "scat" in kw else N, ES[odt]))
    for name, on in (("res", kw.get("res")), ("aux", kw.get("epi")), ("bs_x", kw.get("bstat"))):
        if on:
            d[name] = (N, ES[odt])
    if kw.get("an_out"):
        d["an_out"] = (K, ES[dt])
    return d


def form_params(L, kw, at=None):
    """the miseg_gemm_params of a FORM_ROWS row.  at: name -> (address, row stride) of the real row views and name -> address of the real
    bias / stat / bs_stat / an_stat / workspace / tn_colsum buffers; None: stand-in addresses with each layout's alignment and stride"""
    tn = kw.get("tn", 0)
    dt, odt = dtypes(kw)
    cols = operand_cols(kw)

    def view(name):
        if at is not None:
            return at[name]
        c, es = cols[name]
        off, ld = layout(c, es, kw.get("lay", {}).get(name, "contig"))
        return A + off * es, ld

    def buf(name):
        return at[name] if at is not None else A

    p = L.Gemm()
    (p.A, p.lda), (p.B, p.ldb), (p.C, p.ldc) = view("A"), view("B"), view("C")
    p.M, p.N, p.K, p.ta, p.tb, p.dtype, p.out_dtype = kw["M"], kw["N"], kw["K"], tn, tn, dt, odt
    p.split_k = kw.get("split_k", 0 if tn else 1)
    p.accumulate, p.act, p.epi_mode, p.defer_reduce = kw.get("accumulate", 0), kw.get("act", 0), kw.get("epi", 0), kw.get("defer", 0)
    if kw.get("bias"):
        p.bias = buf("bias")
    if kw.get("res"):
        p.res, p.ldres = view("res")
    if kw.get("epi"):
        p.aux, p.ldaux = view("aux")
    if kw.get("stat") or kw.get("bstat"):
        p.stat = buf("stat")
    if kw.get("bstat"):
        p.stat_mode, p.bs_stat, p.bs_eps = 2, buf("bs_stat"), 1e-5
        p.bs_x, p.ld_bs_x = view("bs_x")
    if kw.get("an"):      # (on the card ops.NormRef.fill writes the styles, gamma and beta rows behind this)
        p.an.stat, p.an.num_styles, p.an.eps = buf("an_stat"), kw["an"], 1e-5
    if kw.get("an_out"):
        p.an_out, p.ld_an_out = view("an_out")
    if "scat" in kw:
        p.scat_d, p.scat_h, p.scat_w, p.scat_cout = kw["scat"]
    if kw.get("colsum"):
        p.tn_colsum = buf("tn_colsum")
    if at is None or "workspace" in at:
        p.workspace = buf("workspace")
    return p


def _f(id_, M, N, K, expect, **kw):
    return (id_, dict(M=M, N=N, K=K, **kw), expect)


FORM_ROWS = []

# ---- the small kernel: a ragged M per tile that keeps the tile (nt_small_tile: the candidate with the most workgroups in 140 .. 256, else
# the first of (2, 4) .. (1, 1) with >= 140, else the last that fits).  Workgroups of the six candidates (4,3) (2,4) (2,2) (2,1) (1,2) (1,1):
#   2041 x 384:  256*  384   768  1536  1536  3072          1727 x 192:  108   162*  324   648   648  1296
#   2047 x  96:   64    -    192*  384   384   768           215 x 384:   32    42    84   168*  168   336      ((2, 1) before (1, 2): first wins a tie)
#    330 x 384:   48    66   132   264   252*  504            27 x 384:    -     6    12    24    24    48*     (none >= 140: the last)
# grid_x: 256 and 192 are multiples of 8, 162 and 252 are not, 48 and the M <= 16 rows' 4 are below the 8 XCDs (the remap at the kernel's top)
SMALL_TILE_ROWS = {
    (4, 3): (2041, 384, dict(grid_x=256, row_tiles=32, col_groups=8, cols_per_group=48)),
    (2, 4): (1727, 192, dict(grid_x=162, row_tiles=54, col_groups=3, cols_per_group=64)),
    (2, 2): (2047, 96, dict(grid_x=192, row_tiles=64, col_groups=3, cols_per_group=32)),
    (2, 1): (215, 384, dict(grid_x=168, row_tiles=7, col_groups=24, cols_per_group=16)),
    (1, 2): (330, 384, dict(grid_x=252, row_tiles=21, col_groups=12, cols_per_group=32)),
    (1, 1): (27, 384, dict(grid_x=48, row_tiles=2, col_groups=24, cols_per_group=16)),
}
SMALL_EPILOGUES = {"plain": ((0, 0, 0), {}), "gelu": ((1, 0, 0), dict(act=GELU)), "anorm": ((0, 0, 1), {}), "anorm-gelu": ((1, 0, 1), dict(act=GELU)),
                   "stat": ((0, 1, 0), dict(stat=1)), "bstat": ((0, 2, 0), dict(bstat=1))}
# K: 32 (three of the four waves have no k-step), 96, 160 (uneven over the waves), 544 (a wave's share is more than one batch of SM_BS
# k-steps), 384 (the folded norm's ncoef limit); every epilogue sees at least two of them
_SMALL = [
    ((4, 3), "plain", 32, "", {}), ((2, 4), "plain", 96, "-bias-a-slice", dict(bias=1, lay=dict(A="slice"))),
    ((2, 2), "plain", 160, "-res-off8", dict(res=1, lay=dict(res="off8"))), ((2, 1), "plain", 544, "-ggrad", dict(epi=2)),
    ((1, 2), "plain", 32, "-c-off8", dict(lay=dict(C="off8"))), ((1, 1), "plain", 544, "-bias-b-slice", dict(bias=1, lay=dict(B="slice"))),
    ((4, 3), "gelu", 96, "-bias-preact-aux-slice", dict(bias=1, epi=1, lay=dict(aux="slice"))), ((2, 4), "gelu", 160, "", {}),
    ((2, 2), "gelu", 544, "-bias-res", dict(bias=1, res=1)), ((2, 1), "gelu", 32, "-c-slice", dict(lay=dict(C="slice"))),
    ((1, 2), "gelu", 96, "-bias-preact", dict(bias=1, epi=1)), ((1, 1), "gelu", 160, "-res-slice", dict(res=1, lay=dict(res="slice"))),
    ((4, 3), "anorm", 160, "-an_out", dict(an=1, an_out=1)), ((2, 4), "anorm", 384, "-styles2-an_out-slice", dict(an=2, an_out=1, lay=dict(an_out="slice"))),
    ((2, 2), "anorm", 32, "-bias", dict(an=1, bias=1)), ((2, 1), "anorm", 96, "-styles4-a-slice", dict(an=4, lay=dict(A="slice"))),
    ((1, 2), "anorm", 384, "-an_out-c-slice", dict(an=1, an_out=1, lay=dict(C="slice"))), ((1, 1), "anorm", 32, "-styles2", dict(an=2)),
    ((4, 3), "anorm-gelu", 32, "-bias-preact-an_out", dict(an=1, bias=1, epi=1, an_out=1)), ((2, 4), "anorm-gelu", 96, "", dict(an=1)),
    ((2, 2), "anorm-gelu", 160, "-styles2-an_out", dict(an=2, an_out=1)), ((2, 1), "anorm-gelu", 384, "-bias", dict(an=1, bias=1)),
    ((1, 2), "anorm-gelu", 160, "-styles4-preact", dict(an=4, epi=1)), ((1, 1), "anorm-gelu", 384, "-an_out-slice", dict(an=1, an_out=1, lay=dict(an_out="slice"))),
    ((4, 3), "stat", 544, "-res", dict(res=1)), ((2, 4), "stat", 32, "-bias", dict(bias=1)), ((2, 2), "stat", 96, "-c-slice", dict(lay=dict(C="slice"))),
    ((2, 1), "stat", 160, "-bias-res-off8", dict(bias=1, res=1, lay=dict(res="off8"))), ((1, 2), "stat", 544, "", {}),
    ((1, 1), "stat", 96, "-a-slice-b-slice", dict(lay=dict(A="slice", B="slice"))),
    ((4, 3), "bstat", 96, "", {}), ((2, 4), "bstat", 544, "-bsx-off8", dict(lay=dict(bs_x="off8"))), ((2, 2), "bstat", 160, "-bias", dict(bias=1)),
    ((2, 1), "bstat", 32, "-bsx-slice", dict(lay=dict(bs_x="slice"))), ((1, 2), "bstat", 160, "-c-slice", dict(lay=dict(C="slice"))),
    ((1, 1), "bstat", 544, "-a-slice", dict(lay=dict(A="slice"))),
]
for (_m, _n), _e, _k, _suffix, _kw in _SMALL:
    _M, _N, _grid = SMALL_TILE_ROWS[(_m, _n)]
    (_g, _s, _a), _req = SMALL_EPILOGUES[_e]
    FORM_ROWS.append(_f("small-%dx%d-%s-m%d-k%d%s" % (_m, _n, _e, _M, _k, _suffix), _M, _N, _k,
                        dict(kernel=SMALL, mtw=_m, ntw=_n, gelu=_g, stat=_s, anorm=_a, **_grid), **dict(_req, **_kw)))
_G4 = dict(grid_x=4, row_tiles=1, col_groups=4, cols_per_group=16)      # M <= 16: no (2, *) tile; (1, 2) 2 and (1, 1) 4 workgroups, the last fits
FORM_ROWS += [
    _f("small-1x1-plain-m1-k32", 1, 64, 32, dict(kernel=SMALL, mtw=1, ntw=1, gelu=0, stat=0, anorm=0, fuses_stat=0, **_G4)),
    _f("small-1x1-plain-m15-k96-bias", 15, 64, 96, dict(kernel=SMALL, mtw=1, ntw=1, fuses_stat=0, fuses_anorm=0, **_G4), bias=1),
    _f("small-1x1-stat-m16-k32", 16, 64, 32, dict(kernel=SMALL, mtw=1, ntw=1, stat=1, fuses_stat=1, **_G4), stat=1),
    _f("small-2x4-plain-ints-m1727-k96", 1727, 192, 96, dict(kernel=SMALL, mtw=2, ntw=4, grid_x=162), ints=1),
]


# ---- the streaming kernel.  grid_x = min(cap, ceil(ceil(M / 32) / 4)): 4101 rows are 129 tiles (the last of 5 rows: its second 16-row half
# is empty) on 33 workgroups = 132 waves, one tile a wave; column groups: the smallest divisor d of N / 16 with 33 d >= 300, else N / 16 -
# 16 columns a group at N = 48 .. 192.  38405 rows: 1201 tiles, 301 workgroups, ONE column group (several accumulator chunks where
# N > 16 nch).  66553 rows: 2080 tiles on the 512-workgroup cap = 2048 waves, 32 of which walk a second tile; 67320 = 2 x 30 x 33 x 34: 2104.
def _st(id_, M, N, K, form, grid, **kw):
    k16, gelu, nch, stat, scat, anorm = form
    gx, gy, cpg = grid
    e = dict(kernel=STREAM, k16=k16, gelu=gelu, nch=nch, stat=stat, scat=scat, anorm=anorm, grid_x=gx, grid_y=gy, col_groups=gy, cols_per_group=cpg)
    e.update(kw.pop("expect", {}))
    return _f(id_, M, N, K, e, **kw)


FORM_ROWS += [
    _st("stream-k3-plain-m4101-n48", 4101, 48, 48, (3, 0, 12, 0, 0, 0), (33, 3, 16), expect=dict(lds_bytes=1856)),
    _st("stream-k3-gelu-m4101-n144-bias-c-off8", 4101, 144, 48, (3, 1, 12, 0, 0, 0), (33, 9, 16), act=GELU, bias=1, lay=dict(C="off8")),
    _st("stream-k6-plain-m4101-n96-a-slice-b-slice-res-off8", 4101, 96, 96, (6, 0, 12, 0, 0, 0), (33, 6, 16), res=1, lay=dict(A="slice", B="slice", res="off8")),
    _st("stream-k6-gelu-m4101-n192-preact-aux-slice", 4101, 192, 96, (6, 1, 12, 0, 0, 0), (33, 12, 16), act=GELU, epi=1, lay=dict(aux="slice")),
    _st("stream-k9-plain-m4101-n48-ggrad", 4101, 48, 144, (9, 0, 12, 0, 0, 0), (33, 3, 16), epi=2),
    _st("stream-k9-gelu-m4101-n96", 4101, 96, 144, (9, 1, 12, 0, 0, 0), (33, 6, 16), act=GELU),
    _st("stream-k12-plain-m4101-n192-c-slice", 4101, 192, 192, (12, 0, 12, 0, 0, 0), (33, 12, 16), lay=dict(C="slice")),
    _st("stream-k12-gelu-m4101-n48-bias", 4101, 48, 192, (12, 1, 12, 0, 0, 0), (33, 3, 16), act=GELU, bias=1),
    _st("stream-k18-plain-m4101-n96", 4101, 96, 288, (18, 0, 6, 0, 0, 0), (33, 6, 16)),
    _st("stream-k18-gelu-m4101-n48-res", 4101, 48, 288, (18, 1, 6, 0, 0, 0), (33, 3, 16), act=GELU, res=1),
    _st("stream-k24-plain-m38405-n96-two-chunks", 38405, 96, 384, (24, 0, 3, 0, 0, 0), (301, 1, 96), bias=1),      # nch 3: chunks of 48 columns
    _st("stream-k24-gelu-m4101-n48", 4101, 48, 384, (24, 1, 3, 0, 0, 0), (33, 3, 16), act=GELU),
    _st("stream-k3-plain-m38405-n384-two-chunks", 38405, 384, 48, (3, 0, 12, 0, 0, 0), (301, 1, 384), bias=1, expect=dict(lds_bytes=44544)),
    _st("stream-k3-plain-ints-m4101-n48", 4101, 48, 48, (3, 0, 12, 0, 0, 0), (33, 3, 16), ints=1),
    _st("stream-k3-anorm-m4101-n144-styles2-an_out-slice", 4101, 144, 48, (3, 0, 12, 0, 0, 1), (33, 9, 16), an=2, an_out=1, lay=dict(an_out="slice")),
    _st("stream-k3-anorm-gelu-m66553-n48-walk-an_out", 66553, 48, 48, (3, 1, 12, 0, 0, 1), (512, 1, 48), an=1, act=GELU, an_out=1, bias=1),
    _st("stream-k6-anorm-m4101-n96-styles4", 4101, 96, 96, (6, 0, 12, 0, 0, 1), (33, 6, 16), an=4),
    _st("stream-k6-anorm-gelu-m4101-n192-preact-an_out", 4101, 192, 96, (6, 1, 12, 0, 0, 1), (33, 12, 16), an=1, act=GELU, epi=1, an_out=1),
    _st("stream-k3-stat-m66553-n48-walk-res", 66553, 48, 48, (3, 0, 6, 1, 0, 0), (512, 1, 48), stat=1, res=1, expect=dict(lds_bytes=24960)),
    _st("stream-k6-stat-m4101-n96-bias", 4101, 96, 96, (6, 0, 6, 1, 0, 0), (33, 6, 16), stat=1, bias=1),
    _st("stream-k12-stat-m4101-n48-c-off8", 4101, 48, 192, (12, 0, 6, 1, 0, 0), (33, 3, 16), stat=1, lay=dict(C="off8")),
    _st("stream-k3-bstat-m66553-n48-walk", 66553, 48, 48, (3, 0, 6, 2, 0, 0), (512, 1, 48), bstat=1),
    _st("stream-k6-bstat-m4101-n96-bsx-off8", 4101, 96, 96, (6, 0, 6, 2, 0, 0), (33, 6, 16), bstat=1, lay=dict(bs_x="off8")),
    _st("stream-k9-bstat-m4101-n48", 4101, 48, 144, (9, 0, 6, 2, 0, 0), (33, 3, 16), bstat=1),
    _st("stream-k12-bstat-m4101-n96-bias", 4101, 96, 192, (12, 0, 6, 2, 0, 0), (33, 6, 16), bstat=1, bias=1),
    # one chunk per column group with the sums: 96 columns over nch 3 = 48 a chunk make two groups
    _st("stream-k18-bstat-m38405-n96-two-groups", 38405, 96, 288, (18, 0, 3, 2, 0, 0), (301, 2, 48), bstat=1, expect=dict(lds_bytes=28992)),
    # 4368 = 2 x 12 x 14 x 13 voxels: 137 tiles on 35 workgroups; the scattered store keeps one column group
    _st("stream-k6-scat-m4368-n384-left-half", 4368, 384, 96, (6, 0, 12, 0, 1, 0), (35, 1, 384), scat=(12, 14, 13, 48), lay=dict(C="left"), expect=dict(lds_bytes=81408)),
    _st("stream-k3-scat-m67320-n64-walk-left-half", 67320, 64, 48, (3, 0, 12, 0, 1, 0), (512, 1, 64), scat=(30, 33, 34, 8), lay=dict(C="left")),
]


# ---- the generic NT kernel: 128 x 16 nt tiles; a stage is 8 chunks of 16 bytes = 64 bf16 / 32 fp32 of K; k_per_split is a multiple of it
def _g(id_, M, N, K, nt, grid, al, kps, mode=STORE, zf=0, **kw):
    e = dict(kernel=NT_GENERIC, nt=nt, grid_x=grid[0], grid_y=grid[1], grid_z=grid[2], splits=grid[2], k_per_split=kps, out_mode=mode, zero_fill=zf, al_a=al[0], al_b=al[1])
    return _f(id_, M, N, K, e, **kw)


F32, BF32 = dict(dt=0), dict(dt=1, odt=0)
_EDGE = dict(M=4101, N=48, K=48, nt=3, grid=(33, 1, 1), kps=64)      # what a-off2 .. ldres-50 of ROWS send to the generic kernel, at 4101 rows
FORM_ROWS += [
    _g("nt1-f32-m129-n12-k22-bias", 129, 12, 22, 1, (2, 1, 1), (0, 0), 32, bias=1, **F32),      # K below one stage, K % 4 != 0: element loads
    _g("nt2-f32-m257-n24-k100-gelu-res", 257, 24, 100, 2, (3, 1, 1), (1, 1), 128, act=GELU, res=1, **F32),
    _g("nt3-f32-m300-n40-k70-gelu-preact", 300, 40, 70, 3, (3, 1, 1), (0, 0), 96, act=GELU, epi=1, bias=1, **F32),
    _g("nt4-f32-m130-n72-k33-ggrad", 130, 72, 33, 4, (2, 2, 1), (0, 0), 64, epi=2, **F32),
    _g("nt4-f32-m129-n64-k64-plain", 129, 64, 64, 4, (2, 1, 1), (1, 1), 64, **F32),      # the 16-byte store of four columns
    _g("nt4-f32-m129-n70-k64-c-ldodd", 129, 70, 64, 4, (2, 2, 1), (1, 1), 64, lay=dict(C="ldodd"), **F32),
    _g("nt1-f32-m129-n12-k36-a-off4", 129, 12, 36, 1, (2, 1, 1), (0, 1), 64, lay=dict(A="off4"), **F32),
    _g("nt4-f32-split4-m200-n64-k300-bias", 200, 64, 300, 4, (2, 1, 4), (1, 1), 96, ATOMIC, 1, split_k=4, bias=1, **F32),
    _g("nt3-f32-split4-acc-m200-n40-k300-bias", 200, 40, 300, 3, (2, 1, 4), (1, 1), 96, ATOMIC, 0, split_k=4, accumulate=1, bias=1, **F32),
    _g("nt2-f32-acc-m129-n20-k100", 129, 20, 100, 2, (2, 1, 1), (1, 1), 128, ACCUMULATE, 0, accumulate=1, **F32),
    # split_k > 1 over a K of one stage: ONE split, so it stores (or accumulates if asked) - DESIGN.md 3.3 (4)
    _g("nt4-f32-split4-one-stage-m64-n64-k32", 64, 64, 32, 4, (1, 1, 1), (1, 1), 32, STORE, 0, split_k=4, **F32),
    _g("nt3-f32-split4-one-stage-m70-n40-k20-bias-c-ldodd", 70, 40, 20, 3, (1, 1, 1), (1, 1), 32, STORE, 0, split_k=4, bias=1, lay=dict(C="ldodd"), **F32),
    _g("nt1-f32-split4-acc-one-stage-m70-n16-k32", 70, 16, 32, 1, (1, 1, 1), (1, 1), 32, ACCUMULATE, 0, split_k=4, accumulate=1, **F32),
    _g("nt3-f32-ints-m70-n33-k40", 70, 33, 40, 3, (1, 1, 1), (1, 1), 64, ints=1, **F32),
    _g("nt1-bf16f32-m129-n12-k20", 129, 12, 20, 1, (2, 1, 1), (0, 0), 64, **BF32),      # K below one stage, K % 8 != 0
    _g("nt2-bf16f32-m257-n24-k104-bias-gelu", 257, 24, 104, 2, (3, 1, 1), (1, 1), 128, bias=1, act=GELU, **BF32),
    _g("nt3-bf16f32-split4-bias-m300-n40-k600-c-ldodd", 300, 40, 600, 3, (3, 1, 4), (1, 1), 192, ATOMIC, 1, split_k=4, bias=1, lay=dict(C="ldodd"), **BF32),
    _g("nt4-bf16f32-split4-acc-m200-n72-k600", 200, 72, 600, 4, (2, 2, 4), (1, 1), 192, ATOMIC, 0, split_k=4, accumulate=1, **BF32),
    _g("nt1-bf16f32-split4-m129-n16-k300", 129, 16, 300, 1, (2, 1, 3), (0, 0), 128, ATOMIC, 1, split_k=4, **BF32),      # 4 asked, 3 of 128 run
    _g("nt2-bf16f32-acc-m129-n32-k72-a-ldodd", 129, 32, 72, 2, (2, 1, 1), (0, 1), 128, ACCUMULATE, 0, accumulate=1, lay=dict(A="ldodd"), **BF32),
    _g("nt4-bf16f32-split4-one-stage-m70-n64-k64", 70, 64, 64, 4, (1, 1, 1), (1, 1), 64, STORE, 0, split_k=4, **BF32),
    _g("nt4-bf16f32-ints-m70-n72-k40", 70, 72, 40, 4, (1, 2, 1), (1, 1), 64, ints=1, **BF32),
    _g("nt1-bf16-m2100-n16-k40-bias", 2100, 16, 40, 1, (17, 1, 1), (1, 1), 64, bias=1),      # 2048 < M < 4096: neither bf16 kernel
    _g("nt2-bf16-m300-n20-k72-gelu-res", 300, 20, 72, 2, (3, 1, 1), (1, 1), 128, act=GELU, res=1),
    _g("nt3-bf16-m300-n40-k100-gelu-preact", 300, 40, 100, 3, (3, 1, 1), (0, 0), 128, act=GELU, epi=1),
    _g("nt4-bf16-m300-n72-k20-ggrad", 300, 72, 20, 4, (3, 2, 1), (0, 0), 64, epi=2),
    _g("nt3-bf16-ints-m70-n33-k40", 70, 33, 40, 3, (1, 1, 1), (1, 1), 64, ints=1),
    _g("nt3-bf16-m4101-a-off2", al=(0, 1), lay=dict(A="off2"), **_EDGE),
    _g("nt3-bf16-m4101-b-off8", al=(1, 0), lay=dict(B="off8"), **_EDGE),
    _g("nt3-bf16-m4101-c-off4", al=(1, 1), lay=dict(C="off4"), **_EDGE),
    _g("nt3-bf16-m4101-res-off4", al=(1, 1), res=1, lay=dict(res="off4"), **_EDGE),
    _g("nt3-bf16-m4101-preact-aux-off4", al=(1, 1), epi=1, lay=dict(aux="off4"), **_EDGE),
    _g("nt3-bf16-m4101-a-ldodd", al=(0, 1), lay=dict(A="ldodd"), **_EDGE),
    _g("nt3-bf16-m4101-b-ldodd", al=(1, 0), lay=dict(B="ldodd"), **_EDGE),
    _g("nt3-bf16-m4101-c-ldodd", al=(1, 1), lay=dict(C="ldodd"), **_EDGE),
    _g("nt3-bf16-m4101-res-ldodd", al=(1, 1), res=1, lay=dict(res="ldodd"), **_EDGE),
]

# ---- rank-1 (K = 1).  Plain: ceil(M (N / n16) / 256) workgroups; with statistics ceil(M / rows) with rows = floor(256 / (N / n16)) a workgroup:
# 42 at 48 bf16 columns (5003 = 119 x 42 + 5), 32 at 32 fp32 columns
FORM_ROWS += [
    _f("rank1-bf16-m5003-n48", 5003, 48, 1, dict(kernel=RANK1, grid_x=118, grid_y=1, grid_z=1, fuses_stat=1)),
    _f("rank1-bf16-bias-m5003-n48-a-slice", 5003, 48, 1, dict(kernel=RANK1, grid_x=118), bias=1, lay=dict(A="slice")),
    _f("rank1-bf16-stat-m5003-n48", 5003, 48, 1, dict(kernel=RANK1_STAT, grid_x=120), stat=1),
    _f("rank1-bf16-stat-bias-m5003-n48-a-slice-c-slice", 5003, 48, 1, dict(kernel=RANK1_STAT, grid_x=120), stat=1, bias=1, lay=dict(A="slice", C="slice")),
    _f("rank1-bf16-stat-m100-n48", 100, 48, 1, dict(kernel=RANK1_STAT, grid_x=3), stat=1),
    _f("rank1-bf16-m1000-n136", 1000, 136, 1, dict(kernel=RANK1, grid_x=67, fuses_stat=0)),
    _f("rank1-bf16-ints-m100-n48", 100, 48, 1, dict(kernel=RANK1, grid_x=3), ints=1),
    _f("rank1-f32-m1000-n32", 1000, 32, 1, dict(kernel=RANK1, grid_x=32, fuses_stat=1), **F32),
    _f("rank1-f32-bias-m1000-n32-a-slice-b-slice", 1000, 32, 1, dict(kernel=RANK1, grid_x=32), bias=1, lay=dict(A="slice", B="slice"), **F32),
    _f("rank1-f32-stat-m1000-n32", 1000, 32, 1, dict(kernel=RANK1_STAT, grid_x=32), stat=1, **F32),
    _f("rank1-f32-stat-bias-m1001-n32-c-slice", 1001, 32, 1, dict(kernel=RANK1_STAT, grid_x=32), stat=1, bias=1, lay=dict(C="slice"), **F32),
    _f("rank1-f32-split4-m1000-n32", 1000, 32, 1, dict(kernel=RANK1, grid_x=32, fuses_stat=0), split_k=4, **F32),
    _f("rank1-f32-stat-ints-m100-n32", 100, 32, 1, dict(kernel=RANK1_STAT, grid_x=4), stat=1, ints=1, **F32),
]


# ---- TN, generic: 64 x 64 tiles; stages of 128 (bf16) / 64 (fp32) reduction rows; the library's split: ceil(K / 512), at most 1024 / tiles
def _t(id_, M, N, K, grid, al, kps, mode=STORE, zf=0, **kw):
    e = dict(kernel=TN_GENERIC, grid_x=grid[0], grid_y=grid[1], grid_z=grid[2], splits=grid[2], k_per_split=kps, out_mode=mode, zero_fill=zf, al_a=al[0], al_b=al[1],
             tn_fuses_colsum=0, workspace_bytes=0)
    return _f(id_, M, N, K, e, tn=1, **kw)


FORM_ROWS += [
    _t("tn-f32-split1-k333-m12-n36", 12, 36, 333, (1, 1, 1), (1, 1), 384, split_k=1, dt=0),
    _t("tn-bf16f32-auto-k1000-m144-n50", 144, 50, 1000, (3, 1, 2), (1, 0), 512, ATOMIC, 1),
    _t("tn-bf16f32-split4-k700-m70-n100", 70, 100, 700, (2, 2, 3), (0, 0), 256, ATOMIC, 1, split_k=4),      # 4 asked, 3 of 256 run
    _t("tn-bf16f32-split4-acc-k700-m72-n104-c-ldodd", 72, 104, 700, (2, 2, 3), (1, 1), 256, ATOMIC, 0, split_k=4, accumulate=1, lay=dict(C="ldodd")),
    _t("tn-f32-acc-split1-k200-m70-n100", 70, 100, 200, (2, 2, 1), (0, 1), 256, ACCUMULATE, 0, split_k=1, accumulate=1, dt=0),
    _t("tn-f32-auto-k1100-m70-n100-a-off4", 70, 100, 1100, (2, 2, 3), (0, 1), 384, ATOMIC, 1, dt=0, lay=dict(A="off4")),
    _t("tn-bf16-split1-k300-m70-n100", 70, 100, 300, (2, 2, 1), (0, 0), 384, split_k=1, odt=1),
    # bf16 output has no atomics: the library's own split stays at one
    _t("tn-bf16-auto-k1000-m72-n104", 72, 104, 1000, (2, 2, 1), (1, 1), 1024, odt=1),
    _t("tn-f32-ints-split1-k100-m50-n70", 50, 70, 100, (1, 2, 1), (0, 0), 128, split_k=1, dt=0, ints=1),
    _t("tn-bf16f32-ints-auto-k1000-m72-n104", 72, 104, 1000, (2, 2, 2), (1, 1), 512, ATOMIC, 1, ints=1),
    # the three refusals of the streaming path, onto this kernel
    _t("tn-stream-k2047", 144, 48, 2047, (3, 1, 4), (1, 1), 512, ATOMIC, 1),
    _t("tn-stream-m40", 40, 48, 2048, (1, 1, 4), (1, 1), 512, ATOMIC, 1),
    _t("tn-stream-a-off8", 144, 48, 2048, (3, 1, 4), (0, 1), 512, ATOMIC, 1, lay=dict(A="off8")),
]


# ---- TN, streaming: 48 x 48 wave tiles as (wm, wn); splits = min(ceil(384 / workgroups), ceil(K / 256)) of whole 64-row stages; reduce groups
# of 16 splits; the partial tiles are splits x M x N floats
def _ts(id_, M, N, K, wave, grid, kps, ws, groups, blocks, mode=STORE, zf=0, **kw):
    e = dict(kernel=TN_STREAM, wm=wave[0], wn=wave[1], grid_x=grid[0], grid_y=grid[1], grid_z=grid[2], splits=grid[2], k_per_split=kps, workspace_bytes=ws,
             reduce_groups=groups, reduce_blocks=blocks, out_mode=mode, zero_fill=zf, tn_fuses_colsum=1, lds_bytes=128 * (96 * (wave[0] + wave[1]) + 32))
    return _f(id_, M, N, K, e, tn=1, **kw)


FORM_ROWS += [
    _ts("tnstream-4x1-k2048-m48-n48-one-group", 48, 48, 2048, (4, 1), (1, 1, 8), 256, 73728, 1, 3),
    _ts("tnstream-4x1-ints-k2048-m48-n48", 48, 48, 2048, (4, 1), (1, 1, 8), 256, 73728, 1, 3, ints=1),
    _ts("tnstream-1x4-k2048-m48-n96-a-slice-b-slice", 48, 96, 2048, (1, 4), (1, 1, 8), 256, 147456, 1, 5, lay=dict(A="slice", B="slice")),
    _ts("tnstream-2x2-k2048-m96-n96-colsum", 96, 96, 2048, (2, 2), (1, 1, 8), 256, 294912, 1, 9, colsum=1),
    _ts("tnstream-2x2-k2048-m96-n96-defer", 96, 96, 2048, (2, 2), (1, 1, 8), 256, 294912, 0, 0, defer=1),
    # 144 rows on two workgroups of 96: the second one's upper waves have no tile
    _ts("tnstream-2x2-k2048-m144-n96-acc-c-slice", 144, 96, 2048, (2, 2), (2, 1, 8), 256, 442368, 1, 14, ACCUMULATE, 0, accumulate=1, lay=dict(C="slice")),
    # 4400 = 17 x 256 + 48: 18 splits, the last one short, two reduce groups that meet in atomics on a filled (or accumulating) C
    _ts("tnstream-4x1-k4400-m144-n48-two-groups-colsum-c-ldodd", 144, 48, 4400, (4, 1), (1, 1, 18), 256, 497664, 2, 7, STORE, 1, colsum=1, lay=dict(C="ldodd")),
    _ts("tnstream-4x1-k4400-m144-n48-two-groups-acc", 144, 48, 4400, (4, 1), (1, 1, 18), 256, 497664, 2, 7, ACCUMULATE, 0, accumulate=1),
    # 400 workgroups: one split, the product goes straight to C
    _ts("tnstream-2x2-k2048-m1920-n1920-one-split", 1920, 1920, 2048, (2, 2), (20, 20, 1), 2048, 0, 0, 0),
    _ts("tnstream-2x2-k2048-m1920-n1920-one-split-acc", 1920, 1920, 2048, (2, 2), (20, 20, 1), 2048, 0, 0, 0, ACCUMULATE, 0, accumulate=1),
]
