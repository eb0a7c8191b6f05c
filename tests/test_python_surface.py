"""The Python package's public surface, pinned: every class and function in habdec_amd.__all__ with its signature and the hash of its docstring, and
for every class each public method and property likewise.  The table was recorded from the package before its plumbing was refactored; a change
that moves a method into a base class, or shares a body, must leave every entry as it is.  No GPU."""
import hashlib
import inspect

import habdec_amd


def _doc(o):
    return None if o.__doc__ is None else hashlib.sha1(o.__doc__.encode()).hexdigest()[:12]


def _sig(o):
    try:
        return str(inspect.signature(o))
    except (TypeError, ValueError):
        return None


def _members(cls):
    out = {}
    for name, m in inspect.getmembers(cls):
        if name.startswith("_"):
            continue
        if isinstance(m, property):
            out[name] = ("property", None, _doc(m))
        elif inspect.isfunction(m):
            out[name] = ("method", _sig(m), _doc(m))
    return out


def surface():
    table = {}
    for name in habdec_amd.__all__:
        o = getattr(habdec_amd, name)
        if inspect.isclass(o):
            table[name] = (_sig(o), _doc(o), _members(o))
        elif inspect.isfunction(o):
            table[name] = (_sig(o), _doc(o), None)
    return table


def test_public_surface_is_unchanged():
    got = surface()
    assert sorted(got) == sorted(SURFACE)
    for name, (sig, doc, members) in SURFACE.items():
        assert got[name][:2] == (sig, doc), name
        if members is not None:
            assert sorted(got[name][2]) == sorted(members), name
            for m, want in members.items():
                assert got[name][2][m] == want, (name, m)


# name: (signature, docstring hash, {member: (kind, signature, docstring hash)} for a class)
SURFACE = {'BaudProbe': ("(eng: 'Engine', **params)",
               'f954f343b1f8',
               {'close': ('method', '(self)', None),
                'estimate': ('method', "(self, s=0) -> 'dict'", None),
                'push_device': ('method', "(self, dev_ptr: 'int', stride: 'int', n_per_stream)", '6a3f4fd040fc'),
                'push_engine': ('method', '(self)', '7f4168346aca'),
                'push_host': ('method', '(self, rows, n_per_stream=None)', None),
                'reset': ('method', '(self, s=None)', None),
                'state': ('method', "(self, s=0) -> 'dict'", None)}),
 'Clocked': ("(eng: 'Engine', **params)",
             '43944a708dbb',
             {'close': ('method', '(self)', None),
              'push_device': ('method', "(self, dev_ptr: 'int', stride: 'int', n_per_stream)", '6a3f4fd040fc'),
              'push_engine': ('method', '(self)', '7f4168346aca'),
              'push_host': ('method', '(self, rows, n_per_stream=None)', None),
              'push_tones': ('method', '(self, tones: "\'Tones\'")', '6df9d7856056'),
              'records': ('method', "(self, s=0, cap=None) -> 'np.ndarray'", 'e3f1a53e340f'),
              'reset': ('method', '(self, s=None)', None),
              'set_modem': ('method', '(self, s, baud, bits, stops, invert=False)', 'f2c54a877f94'),
              'stats': ('method', "(self, s=0) -> 'dict'", None),
              'take_sentences': ('method', "(self, s=0, cap=64) -> 'list'", None),
              'waiting': ('method', "(self, s=0) -> 'int'", None)}),
 'Engine': ("(cfg: 'EngineConfig | None' = None, **kw)",
            None,
            {'afc': ('method', "(self, s=0) -> 'dict'", None),
             'baud_probe': ('method', '(self, **params) -> "\'BaudProbe\'"', '5008cc7aad4a'),
             'bits': ('method', "(self, s=0) -> 'np.ndarray'", None),
             'bits_total': ('method', "(self, s=0) -> 'int'", None),
             'clocked': ('method', '(self, **params) -> "\'Clocked\'"', 'cb53f153094b'),
             'close': ('method', '(self)', None),
             'decimated': ('method', '(self, s=0)', None),
             'demod_checksum': ('method', '(self, s=0)', 'bc537386ab75'),
             'demod_checksum_total': ('method', '(self, s=0)', '0044c4c1f7ee'),
             'demodulated': ('method', '(self, s=0)', None),
             'filtered': ('method', '(self, s=0)', None),
             'fir_taps': ('method', '(self, s=0)', None),
             'flip_list_full': ('method', "(self, s=0) -> 'int'", None),
             'flips': ('method', "(self, s=0) -> 'np.ndarray'", None),
             'flush': ('method', '(self)', None),
             'format_trial': ('method', "(self, s=0) -> 'dict'", None),
             'front_tune': ('method', "(self, s=0) -> 'dict'", None),
             'ingest': ('method', '(self, files: "\'IqFiles\'", max_rounds: \'int\' = 4611686018427387904) -> \'int\'', '633b6b2518d4'),
             'last_sentence': ('method', '(self, s=0)', None),
             'lowpass_taps_max': ('method', "(self) -> 'int'", 'b9b04548f68b'),
             'on_sentence': ('method', '(self, fn)', None),
             'pinned_array': ('method', "(self, shape, dtype=<class 'numpy.complex64'>) -> 'np.ndarray'", '1a28eaa0c557'),
             'power': ('method', '(self, s=0)', None),
             'process_device': ('method', "(self, dev_ptr: 'int', stride: 'int', n: 'int', fmt=None)", '3a99c4a49d0f'),
             'process_host': ('method', "(self, iq: 'np.ndarray', n: 'int | None' = None, fmt=None)", '2ebf7568f79d'),
             'reset_frequency_correction': ('method', '(self, s, c)', None),
             'rtty': ('method', '(self, s=0)', None),
             'sentences_ok': ('method', "(self) -> 'int'", None),
             'set_auto_afc': ('method', '(self, s, on=True, hold_s=6.0, min_hz=100.0)', '860c232e60de'),
             'set_baud': ('method', '(self, s, baud)', None),
             'set_dc_remove': ('method', '(self, s, on)', None),
             'set_format_trial': ('method', '(self, s, on=True)', '278c858af6c6'),
             'set_front_tune': ('method', '(self, s, offset_hz)', 'e5c698594c18'),
             'set_lowpass_bw': ('method', '(self, s, hz)', None),
             'set_lowpass_trans': ('method', '(self, s, t)', None),
             'set_rtty': ('method', '(self, s, bits, stops)', None),
             'set_timing': ('method', "(self, every: 'int')", '41ac0fe9aac5'),
             'set_tune': ('method', '(self, s, offset_hz)', None),
             'spectrum': ('method', '(self, s=0)', None),
             'survey': ('method', '(self) -> "\'Survey\'"', 'ebf785fab64c'),
             'symbol_backlog': ('method', "(self, s=0) -> 'int'", None),
             'take_chars': ('method', '(self, s=0)', None),
             'take_matches': ('method', '(self, s=0)', None),
             'take_sentences': ('method', '(self, s=0)', None),
             'timing': ('method', "(self) -> 'dict'", None),
             'tone_search': ('method', '(self, **params) -> "\'ToneSearch\'"', 'cb46faba7456'),
             'tones': ('method', '(self, **params) -> "\'Tones\'"', 'b21685ec1e7e'),
             'tune': ('method', "(self, s=0) -> 'dict'", None),
             'waterfall': ('method', '(self, **params) -> "\'Waterfall\'"', '1992a5d7a478')}),
 'EngineConfig': ("(n_streams: 'int' = 1, max_chunk: 'int' = 65536, sampling_rate: 'float' = 2048000.0, decimation: 'int' = 64, baud: 'float' = "
                  "300.0, rtty_bits: 'int' = 8, rtty_stops: 'float' = 2.0, lowpass_bw_hz: 'float' = 1500.0, lowpass_trans: 'float' = 0.025, "
                  "dc_remove: 'bool' = False, lookup_mode: 'int' = 1, enable_spectrum: 'bool' = True, ungated: 'bool' = False, keep_filtered: 'bool' "
                  "= False, pipeline: 'int' = 0, arith: 'int' = 0, device: 'int' = 0) -> None",
                  'ba2d9cce4fdd',
                  {}),
 'HabdecError': (None, None, {}),
 'HostBaudProbe': ("(decimated_rate: 'float', **params)",
                   'ed5c7268b4a1',
                   {'close': ('method', '(self)', None),
                    'estimate': ('method', "(self) -> 'dict'", None),
                    'push': ('method', '(self, d)', None),
                    'reset': ('method', '(self)', None),
                    'state': ('method', "(self) -> 'dict'", None)}),
 'HostClocked': ("(decimated_rate: 'float', baud=None, bits=8, stops=2, invert=False, **params)",
                 'ff20aaad47a0',
                 {'close': ('method', '(self)', None),
                  'push': ('method', '(self, d)', None),
                  'records': ('method', "(self, cap=None) -> 'np.ndarray'", None),
                  'reset': ('method', '(self)', None),
                  'set_modem': ('method', '(self, baud, bits, stops, invert=False)', None),
                  'stats': ('method', "(self) -> 'dict'", None),
                  'take_sentences': ('method', "(self, cap=64) -> 'list'", None),
                  'waiting': ('method', "(self) -> 'int'", None)}),
 'HostFormatTrial': ('()',
                     '93b5eebe3999',
                     {'close': ('method', '(self)', None),
                      'get': ('method', "(self) -> 'dict'", None),
                      'push_bits': ('method', '(self, bits)', None)}),
 'HostToneSearch': ('()',
                    'bd0d9368a282',
                    {'close': ('method', '(self)', None),
                     'detect': ('method', "(self, fsd, **params) -> 'dict'", None),
                     'power': ('method', '(self)', None),
                     'push': ('method', '(self, iq)', None),
                     'reset': ('method', '(self)', None)}),
 'HostTones': ("(decimated_rate: 'float', baud=None, f_hi=None, f_lo=None, **params)",
               'ea45528637b3',
               {'close': ('method', '(self)', None),
                'push': ('method', "(self, iq) -> 'np.ndarray'", None),
                'reset': ('method', '(self)', None),
                'set_modem': ('method', '(self, baud, f_hi, f_lo)', None),
                'stats': ('method', "(self) -> 'dict'", None)}),
 'IqFiles': ("(paths, chunk: 'int', granule: 'int', loop: 'bool' = False, realtime_rate: 'float' = 0.0, fmt=None)",
             'd8ff08f3491a',
             {'close': ('method', '(self)', None),
              'count': ('method', "(self, s: 'int') -> 'int'", None),
              'next': ('method', "(self, stride: 'int | None' = None)", 'ca6844270f5d'),
              'next_raw': ('method', "(self, stride: 'int | None' = None)", 'c59f77f2c245'),
              'rewinds': ('method', "(self, s: 'int') -> 'int'", None)}),
 'Survey': ("(eng: 'Engine')",
            '89cd5771c02b',
            {'close': ('method', '(self)', None),
             'detect': ('method', "(self, cap: 'int' = 64, **params) -> 'list'", '5acdb8fe77a4'),
             'power': ('method', '(self)', '16c246129bd5'),
             'push_device': ('method', "(self, dev_ptr: 'int', n: 'int', fmt=None)", 'b5b24120e913'),
             'push_host': ('method', "(self, iq: 'np.ndarray', fmt=None)", 'd3f6c11384e9'),
             'reset': ('method', '(self)', None)}),
 'ToneSearch': ("(eng: 'Engine', **params)",
                '849f78439320',
                {'close': ('method', '(self)', None),
                 'detect': ('method', "(self, s=0, **params) -> 'dict'", 'd15f81fec9a0'),
                 'power': ('method', '(self, s=0)', '2906e9e3dce8'),
                 'push_device': ('method', "(self, dev_ptr: 'int', stride: 'int', n_per_stream)", '94b330b25b5e'),
                 'push_engine': ('method', '(self)', 'b34f0c796474'),
                 'push_host': ('method', '(self, iq, n_per_stream=None)', None),
                 'reset': ('method', '(self, s=None)', None),
                 'stats': ('method', "(self, s=0) -> 'dict'", None)}),
 'Tones': ("(eng: 'Engine', **params)",
           'bc66cc63cc3b',
           {'close': ('method', '(self)', None),
            'output': ('method', "(self, s=0) -> 'np.ndarray'", '20ed9c1597f1'),
            'push_device': ('method', "(self, dev_ptr: 'int', stride: 'int', n_per_stream)", '94b330b25b5e'),
            'push_engine': ('method', '(self)', '21a6c548e124'),
            'push_host': ('method', '(self, iq, n_per_stream=None)', None),
            'reset': ('method', '(self, s=None)', None),
            'rows': ('method', '(self)', '5d641a5d3809'),
            'set_modem': ('method', '(self, s, baud, f_hi, f_lo)', '1c98b7c045e6'),
            'set_modem_from_afc': ('method', '(self, s, baud=0.0)', None),
            'stats': ('method', "(self, s=0) -> 'dict'", None)}),
 'Waterfall': ("(eng: 'Engine', **params)",
               '977f09d5f6d0',
               {'close': ('method', '(self)', None),
                'headers': ('method', "(self, first: 'int' = 0, n: 'int | None' = None) -> 'np.ndarray'", '1292a9800dc8'),
                'hits': ('method', '(self)', '4b1d6b66472d'),
                'marks': ('method', "(self, first: 'int' = 0, n: 'int | None' = None) -> 'np.ndarray'", 'b4aeff3b9d21'),
                'marks_bool': ('method', "(self, first: 'int' = 0, n: 'int | None' = None) -> 'np.ndarray'", '0fce77927206'),
                'push_device': ('method', "(self, dev_ptr: 'int', n: 'int', fmt=None)", '4405a1519615'),
                'push_host': ('method', "(self, iq: 'np.ndarray', fmt=None)", 'd727b9f972ba'),
                'push_rows': ('method', "(self, rows, segments, n_rows: 'int | None' = None)", '24497336b2cf'),
                'reset': ('method', '(self)', None),
                'rows': ('method', "(self, first: 'int', n: 'int', normalised: 'bool' = False) -> 'np.ndarray'", '0fdfb4216e77'),
                'rows_total': ('method', "(self) -> 'int'", None),
                'tracks': ('method', "(self, cap: 'int' = 64, **params) -> 'list'", 'dec8f8a79743')}),
 'chase_repair': ("(span: 'str', data, nbits=8, repair_bits=8, repair_flips=3)", '4a9d073cb332', None),
 'fir_demod_lds_bytes': ("(taps: 'int') -> 'tuple'", '928425e41a4a', None),
 'fir_demod_max_taps': ("(lds_bytes: 'int') -> 'int'", '2fb0e3faad7a', None),
 'lib': ("() -> 'C.CDLL'", '82fc8db882d9', None),
 'survey_detect': ("(power: 'np.ndarray', segments: 'int', sampling_rate: 'float', cap: 'int' = 64, **params) -> 'list'", '452b7a877851', None),
 'tone_search_detect': ("(power: 'np.ndarray', segments: 'int', fsd: 'float', **params) -> 'dict'", '042d7e59e6ef', None),
 'waterfall_tracks': ("(headers: 'np.ndarray', marks: 'np.ndarray', sampling_rate: 'float', cap: 'int' = 64, **params) -> 'list'",
                      'c76f182e9b2d',
                      None)}
