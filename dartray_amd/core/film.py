"""lib/filters/ and lib/film/."""
import math

import numpy as np


class Filter:
    """core/filter.dart:26-39.  ImageFilm tabulates evaluate() at 16 x 16 points (image_film.dart:74-82); the table and
    the two widths are what cross the C ABI (DrFilm.filter_table), so every filter below runs on the device path."""
    def __init__(self, xw, yw):
        self.xWidth = float(xw)
        self.yWidth = float(yw)
        self.invXWidth = 1.0 / self.xWidth
        self.invYWidth = 1.0 / self.yWidth


class BoxFilter(Filter):
    def __init__(self, xw=0.5, yw=0.5):  # box_filter.dart:33-46
        super().__init__(xw, yw)

    def evaluate(self, x, y):
        return 1.0


class GaussianFilter(Filter):
    def __init__(self, xw=2.0, yw=2.0, alpha=2.0):  # gaussian_filter.dart:24-47
        super().__init__(xw, yw)
        self.alpha = float(alpha)
        self.expX = math.exp(-self.alpha * self.xWidth * self.xWidth)
        self.expY = math.exp(-self.alpha * self.yWidth * self.yWidth)

    def _gaussian(self, d, expv):
        return max(0.0, math.exp(-self.alpha * d * d) - expv)

    def evaluate(self, x, y):
        return self._gaussian(x, self.expX) * self._gaussian(y, self.expY)


class MitchellFilter(Filter):
    def __init__(self, b=1.0 / 3.0, c=1.0 / 3.0, xw=2.0, yw=2.0):  # mitchell_filter.dart:24-53
        super().__init__(xw, yw)
        self.b = float(b)
        self.c = float(c)

    def _mitchell1D(self, x):
        b, c = self.b, self.c
        x = abs(2.0 * x)
        if x > 1.0:
            return ((-b - 6 * c) * x * x * x + (6 * b + 30 * c) * x * x + (-12 * b - 48 * c) * x + (8 * b + 24 * c)) * (1.0 / 6.0)
        return ((12 - 9 * b - 6 * c) * x * x * x + (-18 + 12 * b + 6 * c) * x * x + (6 - 2 * b)) * (1.0 / 6.0)

    def evaluate(self, x, y):
        return self._mitchell1D(x * self.invXWidth) * self._mitchell1D(y * self.invYWidth)


class TriangleFilter(Filter):
    def __init__(self, xw=2.0, yw=2.0):  # triangle_filter.dart:24-38
        super().__init__(xw, yw)

    def evaluate(self, x, y):
        return max(0.0, self.xWidth - abs(x)) * max(0.0, self.yWidth - abs(y))


class LanczosSincFilter(Filter):
    def __init__(self, xw=4.0, yw=4.0, tau=3.0):  # lanczos_sinc_filter.dart:24-56
        super().__init__(xw, yw)
        self.tau = float(tau)

    def _sinc1D(self, x):
        x = abs(x)
        if x < 1e-5:
            return 1.0
        if x > 1.0:
            return 0.0
        x *= math.pi
        sinc = math.sin(x) / x
        lanczos = math.sin(x * self.tau) / (x * self.tau)
        return sinc * lanczos

    def evaluate(self, x, y):
        return self._sinc1D(x * self.invXWidth) * self._sinc1D(y * self.invYWidth)


FILTER_TABLE_SIZE = 16  # image_film.dart:307


class ImageFilm:
    def __init__(self, xres, yres, filter=None, cropWindow=(0.0, 1.0, 0.0, 1.0)):
        self.xResolution = int(xres)
        self.yResolution = int(yres)
        self.filter = filter or BoxFilter()
        self.cropWindow = tuple(float(c) for c in cropWindow)
        # image_film.dart:61-65
        self.left = math.ceil(self.xResolution * self.cropWindow[0])
        self.width = max(1, math.ceil(self.xResolution * self.cropWindow[1]) - self.left)
        self.top = math.ceil(self.yResolution * self.cropWindow[2])
        self.height = max(1, math.ceil(self.yResolution * self.cropWindow[3]) - self.top)
        # image_film.dart:74-82
        t = np.zeros(FILTER_TABLE_SIZE * FILTER_TABLE_SIZE, dtype=np.float32)
        fi = 0
        for y in range(FILTER_TABLE_SIZE):
            fy = (y + 0.5) * self.filter.yWidth / FILTER_TABLE_SIZE
            for x in range(FILTER_TABLE_SIZE):
                fx = (x + 0.5) * self.filter.xWidth / FILTER_TABLE_SIZE
                t[fi] = self.filter.evaluate(fx, fy)
                fi += 1
        self.filterTable = t

    def getSampleExtent(self):  # image_film.dart:247-252
        return (math.floor(self.left + 0.5 - self.filter.xWidth),
                math.ceil(self.left + 0.5 + self.width + self.filter.xWidth),
                math.floor(self.top + 0.5 - self.filter.yWidth),
                math.ceil(self.top + 0.5 + self.height + self.filter.yWidth))

    def to_abi(self, f):
        f.xres, f.yres = self.xResolution, self.yResolution
        f.crop[:] = self.cropWindow
        f.filter_xw, f.filter_yw = self.filter.xWidth, self.filter.yWidth
        f.filter_table[:] = [float(v) for v in self.filterTable]
