"""NumPy restatement of the device canvas stream (csrc/synth.hip, DESIGN.md
§4.17): image n of stream `seed` from Philox4x32-10 words in uint64
arithmetic, placed on a float canvas with the pixel test of
datasets.generate_multi_image (no bit masks).  Not collected; the tests
import it."""
import numpy as np

GMAX, ATTEMPTS, RESTARTS, SIDE = 8, 100, 8, 32
QUADS_PER_OBJECT = 1 + ATTEMPTS // 2
QUADS_PER_IMAGE = 4096
STREAM_TAG = 0x53594E54
_M32 = np.uint64(0xFFFFFFFF)


def philox_words(seed: int, ctr, tag: int = STREAM_TAG) -> np.ndarray:
    """[len(ctr), 4] uint64 words (each < 2^32) of Philox4x32-10 with key =
    the halves of `seed` and counter {lo32(ctr), hi32(ctr), tag, 0}."""
    ctr = np.asarray(ctr, np.uint64).reshape(-1)
    c0, c1 = ctr & _M32, ctr >> np.uint64(32)
    c2 = np.full_like(ctr, tag)
    c3 = np.zeros_like(ctr)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2  # 32 x 32 bits: below 2^64
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32)
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1)


def below(word, m: int) -> int:
    return (int(word) * int(m)) >> 32


def synth_ref(bank, sizes, counts, canvas: int, seed: int, first: int, b: int):
    """(images [b, C*C] f32, digits [b] i32, objects [b, 8, 5] i32, status [b]
    i32, stats) of images first .. first + b - 1; stats = {"attempts": the
    accepted attempt number of every object kept, "restarts": per image}."""
    C, G = int(canvas), len(bank)
    images = np.zeros((b, C * C), np.float32)
    digits = np.zeros(b, np.int32)
    objects = np.full((b, GMAX, 5), -1, np.int32)
    status = np.zeros(b, np.int32)
    stats = {"attempts": [], "restarts": np.zeros(b, np.int64)}
    # restart 0 of every image in one pass; later restarts as they are needed
    nq0 = 1 + GMAX * QUADS_PER_OBJECT
    base = (np.arange(b, dtype=np.uint64) + np.uint64(first)) * np.uint64(QUADS_PER_IMAGE)
    first_words = philox_words(
        seed, (base[:, None] + np.arange(nq0, dtype=np.uint64)[None, :]).ravel()).reshape(b, nq0, 4)
    for i in range(b):
        num = int(counts[below(first_words[i, 0, 0], len(counts))])
        for r in range(RESTARTS):
            if r == 0:
                words = first_words[i, 1:]
            else:
                q = 1 + r * GMAX * QUADS_PER_OBJECT + np.arange(GMAX * QUADS_PER_OBJECT)
                words = philox_words(seed, base[i] + q.astype(np.uint64))
            img = np.zeros((C, C), np.float32)
            placed, tried, failed = [], [], False
            for j in range(num):
                blk = words[j * QUADS_PER_OBJECT:(j + 1) * QUADS_PER_OBJECT]
                g = below(blk[0, 0], G)
                h, w = int(sizes[g, 0]), int(sizes[g, 1])
                glyph = bank[g, :h, :w]
                for a in range(ATTEMPTS):
                    x = below(blk[1 + a // 2, 2 * (a % 2)], C - w + 1)
                    y = below(blk[1 + a // 2, 2 * (a % 2) + 1], C - h + 1)
                    if not np.any((glyph > 0) & (img[y:y + h, x:x + w] > 0)):
                        break
                else:
                    failed = True
                    break
                img[y:y + h, x:x + w] += glyph
                placed.append((g, x, y, w, h))
                tried.append(a)
            if not failed:
                break
        stats["restarts"][i] = r
        stats["attempts"] += tried
        images[i] = np.clip(img, 0.0, 1.0).ravel()
        digits[i], status[i] = len(placed), int(failed)
        if placed:
            objects[i, :len(placed)] = placed
    return images, digits, objects, status, stats
