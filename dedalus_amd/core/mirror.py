"""
The host <-> device mirror protocol of every field kind (Cartesian Field, sphere SField, shell ShellField).

A field's authoritative data lives on the device: a coefficient array `_c` and / or a grid array `_g` at `_g_scales`,
`layout` saying which one is current.  `field['g']` / `field['c']` hand out ONE persistent host array in the user's
layout (`_host`, in `_host_layout` at `_host_scales`) that the caller may modify in place, so from that moment the host
copy is the authority (`_authority == "host"`) until the next device use uploads it again (`_sync_to_device`).  This
rule decides whether the user's last write is lost or a stale grid is read, so it is written down once, here.

A field class calls `_init_mirror(dim)` and supplies what really differs between the kinds:

    _user_shape(layout, scales)          shape of the local user array
    _global_shape / _local_slices        only where the user array is distributed (defaults: undistributed)
    _default_scales()                    what `None` scales mean (default: all ones)
    _host_to_device(layout, scales, h)   lay the user array out, upload it, record layout (and scales of grid data)
    _device_to_host(layout, scales)      the inverse: a new user array of the current data
    _forward_transform()                 produce _c from _g (at _g_scales)
    _backward_transform(c, scales)       produce _g, _g_scales from the coefficient array c
    _coeff_array()                       the current coefficient array once layout == "c" (allocated on first use)
"""

import numbers

import numpy as np


def _layout(key):
    return "c" if key in ("c", "coeff") else "g"


class HostMirror:
    # Field sets the scales on the early return of require_grid_space as well; sphere and shell fields do not
    _grid_hit_sets_scales = False

    def _init_mirror(self, dim):
        self.scales = (1.0,) * dim
        # device arrays and which one is current
        self._c = None
        self._g = None
        self._g_scales = None
        self.layout = "c"
        # host mirror
        self._host = None
        self._host_layout = None
        self._host_scales = None
        self._authority = "device"      # 'device' | 'host'

    # ---- defaults of the hooks -------------------------------------------------------------------------------------
    def _default_scales(self):
        return (1.0,) * len(self.scales)

    def _global_shape(self, layout, scales):
        return self._user_shape(layout, scales)

    def _local_slices(self, layout, scales):
        return ()

    def _remedy_scales(self, scales):
        if scales is None:
            return self._default_scales()
        if isinstance(scales, numbers.Number):
            return (float(scales),) * len(self.scales)
        return tuple(float(s) for s in scales)

    # ---- device side ---------------------------------------------------------------------------------------------------
    def _sync_to_device(self):
        """Upload the host mirror if the user may have touched it."""
        if self._authority != "host":
            return
        self._authority = "device"
        self._host_to_device(self._host_layout, self._host_scales, self._host)

    def require_coeff_space(self):
        """Device coefficient array, current (read-only for the caller)."""
        self._sync_to_device()
        if self.layout == "g":
            self._forward_transform()
            self.layout = "c"
        return self._coeff_array()

    def require_grid_space(self, scales=None):
        self._sync_to_device()
        scales = self._remedy_scales(scales)
        if self.layout == "g" and self._g_scales == scales:
            if self._grid_hit_sets_scales:
                self.scales = scales
            return self._g
        self._backward_transform(self.require_coeff_space(), scales)
        self.layout = "g"
        self.scales = scales
        return self._g

    # ---- user access ---------------------------------------------------------------------------------------------------
    def change_scales(self, scales):
        scales = self._remedy_scales(scales)
        if scales == self.scales:
            return
        self._sync_to_device()
        if self.layout == "g":              # (never a constant sphere field: its layout stays "c", it has no transform)
            self.require_coeff_space()
        self.scales = scales

    preset_scales = change_scales

    def __getitem__(self, key):
        if isinstance(key, tuple):
            layout, scales = key
            self.change_scales(scales)
        else:
            layout = key
        layout = _layout(layout)
        if not (self._authority == "host" and self._host_layout == layout
                and (layout == "c" or self._host_scales == self.scales)):
            self._sync_to_device()
            self._host = self._device_to_host(layout, self.scales)
            self._host_layout, self._host_scales = layout, self.scales
        # the caller may modify the mirror in place: the host copy is authoritative from now on
        self._authority = "host"
        return self._host

    def __setitem__(self, key, data):
        if isinstance(key, tuple):
            layout, scales = key
            self.scales = self._remedy_scales(scales)
        else:
            layout = key
        layout = _layout(layout)
        shape = self._user_shape(layout, self.scales)
        if self._host is None or self._host.shape != shape or data is not self._host:
            host = np.empty(shape)
            host[...] = data
            self._host = host
        self._host_layout, self._host_scales = layout, self.scales
        self._authority = "host"

    @property
    def data(self):
        return self[self.layout if self._authority == "device" else self._host_layout]

    def fill_random(self, layout=None, scales=None, seed=None, chunk_size=2 ** 20, distribution="standard_normal", **kw):
        """Reproducible random data: the same global stream the reference draws
        (core/field.py:898-943, tools/random_arrays.py:7-55: chunks of min(size, chunk_size) from
        default_rng(seed), C-ordered over (tensor components, global shape)); every rank keeps its local slices."""
        if scales is not None:
            self.change_scales(scales)
        layout = _layout(layout or self.layout)
        shape = self._global_shape(layout, self.scales)
        n = int(np.prod(shape))
        cs = min(n, chunk_size)
        rng = np.random.default_rng(seed)
        draw = getattr(rng, distribution)
        out = np.empty(n)
        pos = 0
        while pos < n:
            chunk = draw(size=cs, **kw)
            m = min(cs, n - pos)
            out[pos:pos + m] = chunk[:m]
            pos += m
        self[layout] = out.reshape(shape)[self._local_slices(layout, self.scales)]
