/* bk_hostmod_driver.inc -- appended to the generated lens code when it is compiled for the host (bk_lens.cpp: host module).
 * Entry points of the re-derivation of flagged entries: the same per-entry functions the build kernels call
 * (bk_build_kernels.h), on the platform libm.  One BkState per call: script globals a callback assigns are carried from one
 * entry of the run to the next, as the reference's sequential scan carries them (ascending ids: its scan order). */
extern "C" int bk_hostmod_abi(void) { return 5 + (int)sizeof(BkBuildParams) * 16; }

/* The whole inverse build the way the reference runs it (fisheye.c:2084-2124): ONE evaluator state, rows from the bottom up, pixels
 * left to right, stopping at the first malformed result.  off / tint / sub arrive filled with NULL / 255 / 0x8080.  Returns the error bits. */
extern "C" int bk_hostmod_inverse_scan(const BkBuildParams *P, unsigned int *off, unsigned char *tint, unsigned short *sub, int *display)
{
#ifdef BK_HAS_INVERSE
    BkState S;
    bk_state_init(S, P);
    for (int lyl = P->rows - 1; lyl >= 0; --lyl)
        for (int lx = 0; lx < P->W; ++lx) {
            const unsigned long o = (unsigned long)lyl * (unsigned long)P->W + (unsigned long)lx;
            int shown;
            S.err = 0; S.steps = 0; S.flag = 0;
            bk_inverse_entry(*P, S, lx, P->row0 + lyl, &off[o], &tint[o], &shown, &sub[o]);
            if (S.err) { off[o] = 0xFFFFFFFFu; tint[o] = 255; sub[o] = 0x8080; return S.err; }
            if (shown >= 0) display[shown] = 1;
        }
    return 0;
#else
    (void)P; (void)off; (void)tint; (void)sub; (void)display;
    return 0;
#endif
}

extern "C" void bk_hostmod_inverse(const BkBuildParams *P, const unsigned int *rec, int rec_stride, unsigned long n, unsigned int *off,
                                   unsigned char *tint, unsigned short *sub, int *shown, int *err)
{
#ifdef BK_HAS_INVERSE
    BkState S;
    bk_state_init(S, P);
    for (unsigned long i = 0; i < n; ++i) {
        const unsigned int o = rec[i * (unsigned long)rec_stride];
        const int lyl = (int)(o / (unsigned int)P->W), lx = (int)(o - (unsigned int)lyl * (unsigned int)P->W);
        S.err = 0; S.steps = 0; S.flag = 0;
        bk_inverse_entry(*P, S, lx, P->row0 + lyl, &off[i], &tint[i], &shown[i], &sub[i]);
        err[i] = S.err;
    }
#else
    (void)P; (void)rec; (void)rec_stride; (void)n; (void)off; (void)tint; (void)sub; (void)shown; (void)err;
#endif
}

extern "C" void bk_hostmod_corners(const BkBuildParams *P, const unsigned int *rec, int rec_stride, unsigned long n, int *sx, int *sy,
                                   unsigned char *ok, int *err)
{
#ifdef BK_HAS_FORWARD
    BkState S;
    bk_state_init(S, P);
    for (unsigned long i = 0; i < n; ++i) {
        S.err = 0; S.steps = 0; S.flag = 0;
        bk_corner_entry(*P, S, (long long)rec[i * (unsigned long)rec_stride], &sx[i], &sy[i], &ok[i]);
        err[i] = S.err;
    }
#else
    (void)P; (void)rec; (void)rec_stride; (void)n; (void)sx; (void)sy; (void)ok; (void)err;
#endif
}

extern "C" void bk_hostmod_texel_owns(const BkBuildParams *P, const unsigned int *rec, int rec_stride, unsigned long n, unsigned char *own)
{
#ifdef BK_HAS_FORWARD
    BkState S;
    bk_state_init(S, P);
    for (unsigned long i = 0; i < n; ++i) {
        S.err = 0; S.steps = 0; S.flag = 0;
        own[i] = bk_texel_owns(*P, S, (long long)rec[i * (unsigned long)rec_stride]) ? 1 : 0;
    }
#else
    (void)P; (void)rec; (void)rec_stride; (void)n; (void)own;
#endif
}
