"""The candidate lists of one shrink step (TEST INFRASTRUCTURE ONLY): a numpy restatement of the
lists Adversary.shrink builds, level by level and in its order, which psg_shrink_* enumerates on
the device. tests/test_shrink_rule.py pins it to the batches shrink() really evaluates."""
import numpy as np

from round_amd import abi, schedules as S


def candidates(ho, crash, level, arg, n, R, self_bit=True):
    """(hos uint64 [K][R][n][W], crashes int32 [K][n] or None) of the base (ho [R][n][W], crash [n]
    or None). TAIL: arg = check point; LINK: arg = max_candidates (0: no cap); CRASH: arg unused
    (the self bit is `self_bit`). Below CRASH every candidate keeps the base's crash rounds."""
    W = S.words(n)
    fm = S.full_mask(n)
    ho = np.asarray(ho, np.uint64).reshape(R, n, W)
    out, out_c = [], None
    if level == abi.PSG_SHRINK_TAIL:
        h2 = ho.copy()
        h2[arg:] = fm
        out.append(h2)
    elif level == abi.PSG_SHRINK_ROUND:
        for k in range(R):
            if (ho[k] != fm).any():
                h2 = ho.copy()
                h2[k] = fm
                out.append(h2)
    elif level == abi.PSG_SHRINK_SET:
        for k in range(R):
            for p in range(n):
                if (ho[k, p] != fm).any():
                    h2 = ho.copy()
                    h2[k, p] = fm
                    out.append(h2)
    elif level == abi.PSG_SHRINK_LINK:
        done = False
        for k in range(R):
            for p in range(n):
                for q in range(n):
                    if not (int(ho[k, p, q >> 6]) >> (q & 63)) & 1:
                        h2 = ho.copy()
                        h2[k, p, q >> 6] |= np.uint64(1 << (q & 63))
                        out.append(h2)
                if arg and len(out) > arg:
                    done = True
                    break
            if done:
                break
    elif level == abi.PSG_SHRINK_CRASH:
        crash = np.asarray(crash, np.int32)
        cc = []
        for q in np.nonzero(crash >= 0)[0]:
            c2 = crash.copy()
            c2[q] = -1
            cc.append(c2)
        for q in np.nonzero(crash >= 0)[0]:
            if crash[q] + 1 < R:
                c2 = crash.copy()
                c2[q] += 1
                cc.append(c2)
        if not cc:
            return np.zeros((0, R, n, W), np.uint64), np.zeros((0, n), np.int32)
        out_c = np.stack(cc)
        part = np.zeros((len(cc), n, W), np.uint64)
        for q in range(n):
            if crash[q] >= 0:
                part[:, :, q >> 6] |= ho[crash[q]][:, q >> 6] & np.uint64(1 << (q & 63))
        return S.crash_to_ho(out_c, part, R, n, self_bit), out_c
    else:
        raise ValueError(level)
    hos = np.stack(out) if out else np.zeros((0, R, n, W), np.uint64)
    if crash is not None:
        out_c = np.repeat(np.asarray(crash, np.int32)[None], len(hos), 0)
    return hos, out_c


def same_cex(a, b):
    """Two adversary.Counterexample are the same, bit for bit."""
    return a.same(b)
