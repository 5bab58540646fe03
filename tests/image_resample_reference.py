"""Host restatement of ``tg_image_resample_u8``: Pillow's two 8-bit passes in numpy, driven by ``preprocess.resample_plan``'s tables.  The horizontal pass
runs first and rounds to uint8, then the vertical pass; a pass is ``clip8((2^21 + sum p * k) >> 22)`` in integer arithmetic (int64 here: the plan
asserts that int32 would do).  ``pil_resize`` is the reference it is compared with; the GPU tests compare the kernel with both."""
import numpy as np

from theatergen_amd import preprocess

SHAPES = [((200, 232), (800, 928)), ((64, 64), (128, 128)), ((97, 131), (40, 53)), ((512, 512), (1024, 1024)), ((300, 50), (77, 13)),
          ((37, 61), (37, 200)), ((640, 480), (333, 250))]                           # (h, w) -> (h, w): the seven shapes the contract was checked at
EDGE_SHAPES = [((1, 1), (5, 3)), ((5, 3), (1, 1)), ((53, 89), (131, 47))]           # clamping at both borders; a prime-sized pair
FILTERS = {"bilinear": preprocess.BILINEAR, "bicubic": preprocess.BICUBIC}


def one_pass(img, plan, axis):
    """img uint8 [..]: resample ``axis`` with ``plan``"""
    a = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((plan.out_size,) + a.shape[1:], np.int64)
    for i in range(plan.out_size):
        f, c = int(plan.first[i]), int(plan.count[i])
        k = plan.k[i, :c].astype(np.int64).reshape((c,) + (1,) * (a.ndim - 1))
        out[i] = ((1 << (preprocess.PRECISION_BITS - 1)) + (a[f:f + c] * k).sum(0)) >> preprocess.PRECISION_BITS
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def resize(img, out_hw, filter):
    """img uint8 [h, w, 3] -> uint8 [out_h, out_w, 3]"""
    h, w = img.shape[:2]
    horizontal = one_pass(img, preprocess.resample_plan(w, out_hw[1], filter), 1)
    return one_pass(horizontal, preprocess.resample_plan(h, out_hw[0], filter), 0)


def pil_resize(img, out_hw, filter):
    from PIL import Image
    return np.array(Image.fromarray(img).resize((out_hw[1], out_hw[0]), resample=filter))


def random_image(hw, seed):
    return np.random.RandomState(seed).randint(0, 256, (hw[0], hw[1], 3)).astype(np.uint8)


def size_sweep():
    """(h, w) pairs for the size rules: square, portrait, landscape, ties at .5 of the SAM rule (h * 1024 / w ends in .5), the 1333 cap of the
    GroundingDINO rule (aspect ratios beyond 1333 / 800) and sizes around it"""
    pairs = [(512, 512), (1024, 1024), (200, 232), (232, 200), (97, 131), (480, 640), (640, 480), (1, 1), (1, 7), (7, 1), (37, 61), (800, 1333),
             (1333, 800), (800, 1334), (400, 667), (300, 1000), (1000, 300), (50, 300), (333, 250), (799, 1332), (801, 1335), (3, 2048), (2048, 3)]
    pairs += [(h, 2048) for h in (1, 3, 5, 7, 1001, 1023)] + [(2048, w) for w in (1, 3, 5, 999)]          # h * 1024 / 2048 = h / 2: ties for odd h
    pairs += [(h, 4096) for h in (2, 6, 10, 1002)]                                                        # h / 4: ties at h = 2 mod 4
    rs = np.random.RandomState(7)
    pairs += [tuple(int(v) for v in rs.randint(1, 1500, 2)) for _ in range(60)]
    return pairs
