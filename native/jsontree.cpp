// _jsontree: native walks over wire-format JSON trees (dict/list/scalars).
//
// The controller stack spends about a third of its time in three pure tree
// walks: the deep copy every client call returns, the RFC 7386 merge patch,
// and CRD schema validation on every write. This module implements them
// against the raw CPython C API (no binding layer: these run tens of
// thousands of times per second, so per-call overhead matters).
//
//   deep_copy(obj)                  kube/objects.py: deep_copy
//   json_merge_patch(target, patch) kube/client.py: json_merge_patch
//   merge_patch_owned(cur, patch)   == deep_copy(json_merge_patch(cur, patch))
//                                   but shares every untouched subtree of cur
//   crd_valid(schema, new, old, spec_immutable)
//                                   verdict-only kube/crdschema.py walk
//
// The pure-Python functions stay in the package as the fallback and as the
// reference the tests compare against.
#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include "jsontree_walk.h"

namespace {

// the copy and merge walks themselves live in jsontree_walk.h
using jsontree_walk::copy_tree;
using jsontree_walk::merge;
using jsontree_walk::merge_owned;

PyObject* py_deep_copy(PyObject*, PyObject* obj) { return copy_tree(obj); }

PyObject* py_json_merge_patch(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError, "json_merge_patch(target, patch) takes 2 arguments");
        return nullptr;
    }
    return merge(args[0], args[1], false);
}

PyObject* str_metadata;  // interned "metadata"

PyObject* py_merge_patch_owned(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 2) {
        PyErr_SetString(PyExc_TypeError, "merge_patch_owned(cur, patch) takes 2 arguments");
        return nullptr;
    }
    return merge_owned(args[0], args[1], str_metadata);
}

// ---------------------------------------------------------------------------
// CRD validation, verdict only
// ---------------------------------------------------------------------------
//
// Mirrors kube/crdschema.py _validate / _validate_changed / CRDValidator.
// Results: 1 valid, 0 not valid, -1 Python exception set. Only "valid" has
// to be exact: on anything else the caller re-runs the Python validator,
// which produces the messages (or raises). So every shape this walk does not
// mirror exactly (a schema node that is not a plain dict, a dict/list/str
// subclass in the object, a raw uncompiled pattern) answers "not valid".

struct Names {
    PyObject *type, *properties, *additionalProperties, *preserve, *required, *items,
        *maxItems, *enum_set, *enum_, *pattern_re, *pattern, *maxLength, *minLength,
        *minimum, *maximum, *anyOf, *search, *spec, *status, *nodeClassRef, *group,
        *kind, *name, *empty;
} S;

// schema.get(key): borrowed, nullptr when absent (no error: str keys)
inline PyObject* sget(PyObject* schema, PyObject* key) {
    PyObject* v = PyDict_GetItemWithError(schema, key);
    if (v == nullptr) PyErr_Clear();
    return v;
}

// a string validator of an anyOf string branch: the enclosing schema's
// value wins when it has the field (the Python code builds a merged dict)
inline PyObject* sget2(PyObject* schema, PyObject* overlay, PyObject* key) {
    if (overlay != nullptr) {
        PyObject* v = sget(overlay, key);
        if (v != nullptr) return v;
    }
    return sget(schema, key);
}

inline bool is_str(PyObject* o, const char* s) {
    return o != nullptr && PyUnicode_CheckExact(o) && PyUnicode_CompareWithASCIIString(o, s) == 0;
}

// len > limit / len < limit with Python's own comparison
int len_cmp(Py_ssize_t n, PyObject* limit, int op) {
    PyObject* pn = PyLong_FromSsize_t(n);
    if (pn == nullptr) return -1;
    int r = PyObject_RichCompareBool(pn, limit, op);
    Py_DECREF(pn);
    return r;
}

int validate(PyObject* obj, PyObject* schema, PyObject* overlay);

// the object branch's walk over obj, shared by validate() (old == nullptr)
// and validate_changed() (old is the previous revision's dict)
int validate_changed(PyObject* nw, PyObject* old, PyObject* schema);

int check_required(PyObject* obj, PyObject* schema) {
    PyObject* req = sget(schema, S.required);
    if (req == nullptr) return 1;
    if (!PyList_CheckExact(req) && !PyTuple_CheckExact(req)) return 0;
    Py_ssize_t n = PySequence_Fast_GET_SIZE(req);
    for (Py_ssize_t i = 0; i < n; i++) {
        int has = PyDict_Contains(obj, PySequence_Fast_GET_ITEM(req, i));
        if (has <= 0) return has;
    }
    return 1;
}

int validate_string(PyObject* obj, PyObject* schema, PyObject* overlay) {
    if (!PyUnicode_Check(obj)) return 0;
    if (!PyUnicode_CheckExact(obj)) return 0;  // subclass: leave to Python
    PyObject* enum_set = sget2(schema, overlay, S.enum_set);
    if (enum_set != nullptr && enum_set != Py_None) {
        int in = PySequence_Contains(enum_set, obj);
        if (in <= 0) return in;
    } else {
        PyObject* en = sget2(schema, overlay, S.enum_);
        if (en != nullptr) {
            int in = PySequence_Contains(en, obj);
            if (in <= 0) return in;
        }
    }
    PyObject* pat = sget2(schema, overlay, S.pattern_re);
    if (pat != nullptr && pat != Py_None) {
        PyObject* m = PyObject_CallMethodOneArg(pat, S.search, obj);
        if (m == nullptr) return -1;
        bool miss = m == Py_None;
        Py_DECREF(m);
        if (miss) return 0;
    } else if (sget2(schema, overlay, S.pattern) != nullptr) {
        return 0;  // uncompiled pattern: leave to Python
    }
    PyObject* lim = sget2(schema, overlay, S.maxLength);
    if (lim != nullptr) {
        int r = len_cmp(PyUnicode_GET_LENGTH(obj), lim, Py_GT);
        if (r != 0) return r < 0 ? -1 : 0;
    }
    lim = sget2(schema, overlay, S.minLength);
    if (lim != nullptr) {
        int r = len_cmp(PyUnicode_GET_LENGTH(obj), lim, Py_LT);
        if (r != 0) return r < 0 ? -1 : 0;
    }
    return 1;
}

int validate_object(PyObject* obj, PyObject* schema) {
    if (!PyDict_Check(obj)) return 0;
    if (!PyDict_CheckExact(obj)) return 0;  // subclass: leave to Python
    PyObject* props = sget(schema, S.properties);
    PyObject* ap = sget(schema, S.additionalProperties);
    if (ap == Py_None) ap = nullptr;
    if (ap != nullptr && PyDict_Check(ap) && !PyDict_CheckExact(ap)) return 0;
    bool ap_schema = ap != nullptr && PyDict_CheckExact(ap);
    int props_true = props == nullptr ? 0 : PyObject_IsTrue(props);
    if (props_true < 0) return -1;
    if (props_true && !PyDict_CheckExact(props)) return 0;
    if (props_true || ap_schema) {
        bool extra_ok = ap != nullptr;
        if (props_true && !extra_ok) {
            PyObject* pu = sget(schema, S.preserve);
            int t = pu == nullptr ? 0 : PyObject_IsTrue(pu);
            if (t < 0) return -1;
            extra_ok = t != 0;
        }
        Py_ssize_t pos = 0;
        PyObject *k, *v;
        while (PyDict_Next(obj, &pos, &k, &v)) {
            PyObject* sub = nullptr;
            if (props_true) {
                sub = PyDict_GetItemWithError(props, k);
                if (sub == nullptr && PyErr_Occurred()) return -1;
                if (sub == Py_None) sub = nullptr;
            }
            if (sub == nullptr && ap_schema) sub = ap;
            if (sub == nullptr) {
                if (!extra_ok) return 0;  // unknown field
                continue;
            }
            if (!PyDict_CheckExact(sub)) return 0;
            int r = validate(v, sub, nullptr);
            if (r <= 0) return r;
        }
    }
    return check_required(obj, schema);
}

int validate_any_of(PyObject* obj, PyObject* schema, PyObject* branches) {
    if (!PyList_CheckExact(branches)) return 0;
    bool string_fields = sget(schema, S.pattern) || sget(schema, S.pattern_re) ||
                         sget(schema, S.maxLength) || sget(schema, S.minLength) ||
                         sget(schema, S.enum_);
    for (Py_ssize_t i = 0; i < PyList_GET_SIZE(branches); i++) {
        PyObject* b = PyList_GET_ITEM(branches, i);
        if (!PyDict_CheckExact(b)) return 0;
        PyObject* overlay = nullptr;
        if (string_fields && is_str(sget(b, S.type), "string")) overlay = schema;
        int r = validate(obj, b, overlay);
        if (r != 0) return r;  // matched, or error
    }
    return 0;
}

int validate(PyObject* obj, PyObject* schema, PyObject* overlay) {
    if (Py_EnterRecursiveCall(" while validating against a CRD schema")) return -1;
    int r = 1;
    PyObject* t = sget(schema, S.type);
    if (t != nullptr && t != Py_None && !PyUnicode_CheckExact(t)) {
        r = 0;
    } else if (is_str(t, "object") ||
               ((t == nullptr || t == Py_None) && sget(schema, S.properties) != nullptr)) {
        r = validate_object(obj, schema);
    } else if (is_str(t, "array")) {
        if (!PyList_CheckExact(obj)) {
            r = 0;
        } else {
            PyObject* lim = sget(schema, S.maxItems);
            if (lim != nullptr) {
                int c = len_cmp(PyList_GET_SIZE(obj), lim, Py_GT);
                if (c != 0) r = c < 0 ? -1 : 0;
            }
            PyObject* items = sget(schema, S.items);
            int items_true = (r == 1 && items != nullptr) ? PyObject_IsTrue(items) : 0;
            if (items_true < 0) r = -1;
            if (r == 1 && items_true) {
                if (!PyDict_CheckExact(items)) r = 0;
                for (Py_ssize_t i = 0; r == 1 && i < PyList_GET_SIZE(obj); i++)
                    r = validate(PyList_GET_ITEM(obj, i), items, nullptr);
            }
        }
    } else if (is_str(t, "string")) {
        r = validate_string(obj, schema, overlay);
    } else if (is_str(t, "integer")) {
        if (!PyLong_Check(obj) || PyBool_Check(obj)) {
            r = 0;
        } else {
            PyObject* lim = sget(schema, S.minimum);
            if (lim != nullptr) {
                int c = PyObject_RichCompareBool(obj, lim, Py_LT);
                if (c != 0) r = c < 0 ? -1 : 0;
            }
            lim = sget(schema, S.maximum);
            if (r == 1 && lim != nullptr) {
                int c = PyObject_RichCompareBool(obj, lim, Py_GT);
                if (c != 0) r = c < 0 ? -1 : 0;
            }
        }
    } else if (is_str(t, "boolean")) {
        if (!PyBool_Check(obj)) r = 0;
    }
    if (r == 1) {
        PyObject* any_of = sget(schema, S.anyOf);
        if (any_of != nullptr)
            r = overlay != nullptr ? 0 : validate_any_of(obj, schema, any_of);
    }
    Py_LeaveRecursiveCall();
    return r;
}

// _validate_changed: only what differs from the previous revision is
// walked; identity prunes in O(1), equality prunes the rest.
int validate_changed(PyObject* nw, PyObject* old, PyObject* schema) {
    if (nw == old) return 1;
    if (Py_EnterRecursiveCall(" while validating against a CRD schema")) return -1;
    int r = 1;
    PyObject* props = sget(schema, S.properties);
    if (props == Py_None) props = nullptr;
    PyObject* items = sget(schema, S.items);
    if ((PyDict_Check(nw) && !PyDict_CheckExact(nw)) || (PyDict_Check(old) && !PyDict_CheckExact(old)) ||
        (PyList_Check(nw) && !PyList_CheckExact(nw)) || (PyList_Check(old) && !PyList_CheckExact(old)) ||
        (props != nullptr && !PyDict_CheckExact(props)) ||
        (items != nullptr && PyDict_Check(items) && !PyDict_CheckExact(items))) {
        r = 0;  // subclasses: leave to Python
    } else if (PyDict_CheckExact(nw) && PyDict_CheckExact(old) && props != nullptr) {
        PyObject* ap = sget(schema, S.additionalProperties);
        if (ap == Py_None) ap = nullptr;
        bool ap_schema = ap != nullptr && PyDict_CheckExact(ap);
        if (ap != nullptr && PyDict_Check(ap) && !ap_schema) r = 0;
        bool extra_ok = ap != nullptr;
        if (r == 1 && !extra_ok) {
            PyObject* pu = sget(schema, S.preserve);
            int t = pu == nullptr ? 0 : PyObject_IsTrue(pu);
            if (t < 0) r = -1;
            extra_ok = t > 0;
        }
        bool props_true = PyDict_GET_SIZE(props) > 0;
        Py_ssize_t pos = 0;
        PyObject *k, *v;
        while (r == 1 && PyDict_Next(nw, &pos, &k, &v)) {
            PyObject* sub = PyDict_GetItemWithError(props, k);
            if (sub == nullptr && PyErr_Occurred()) { r = -1; break; }
            if (sub == Py_None) sub = nullptr;
            if (sub == nullptr && ap_schema) sub = ap;
            if (sub == nullptr) {
                if (props_true && !extra_ok) r = 0;  // unknown field
                continue;
            }
            if (!PyDict_CheckExact(sub)) { r = 0; break; }
            PyObject* ov = PyDict_GetItemWithError(old, k);
            if (ov == nullptr && PyErr_Occurred()) { r = -1; break; }
            r = ov == nullptr ? validate(v, sub, nullptr) : validate_changed(v, ov, sub);
        }
        if (r == 1) r = check_required(nw, schema);
    } else if (PyList_CheckExact(nw) && PyList_CheckExact(old) && items != nullptr &&
               PyDict_CheckExact(items)) {
        PyObject* lim = sget(schema, S.maxItems);
        if (lim != nullptr) {
            int c = len_cmp(PyList_GET_SIZE(nw), lim, Py_GT);
            if (c != 0) r = c < 0 ? -1 : 0;
        }
        // an element equal to any previously stored element was already
        // validated (a conditions write touches one entry)
        for (Py_ssize_t i = 0; r == 1 && i < PyList_GET_SIZE(nw); i++) {
            PyObject* item = PyList_GET_ITEM(nw, i);
            Py_INCREF(item);
            int seen = 0;
            for (Py_ssize_t j = 0; seen == 0 && j < PyList_GET_SIZE(old); j++) {
                PyObject* o = PyList_GET_ITEM(old, j);
                Py_INCREF(o);
                seen = PyObject_RichCompareBool(item, o, Py_EQ);
                Py_DECREF(o);
            }
            if (seen < 0) r = -1;
            else if (seen == 0) r = validate(item, items, nullptr);
            Py_DECREF(item);
        }
    } else {
        int eq = PyObject_RichCompareBool(nw, old, Py_EQ);
        if (eq < 0) r = -1;
        else if (eq == 0) r = validate(nw, schema, nullptr);
    }
    Py_LeaveRecursiveCall();
    return r;
}

// CRDValidator.__call__ without _apply_defaults (which stays in Python and
// has already run on create)
int crd_valid(PyObject* schema, PyObject* nw, PyObject* old, bool spec_immutable) {
    if (!PyDict_CheckExact(schema) || !PyDict_CheckExact(nw)) return 0;
    PyObject* spec = sget(nw, S.spec);
    if (old == Py_None) {
        int r = validate(nw, schema, nullptr);
        if (r <= 0) return r;
    } else {
        if (!PyDict_CheckExact(old)) return 0;
        PyObject* props = sget(schema, S.properties);
        if (props != nullptr && !PyDict_CheckExact(props)) return 0;
        PyObject* keys[2] = {S.spec, S.status};
        for (PyObject* key : keys) {
            PyObject* ns = sget(nw, key);
            PyObject* olds = sget(old, key);
            PyObject* sub = props ? sget(props, key) : nullptr;
            if (sub == nullptr || sub == Py_None || ns == nullptr || ns == Py_None) continue;
            if (!PyDict_CheckExact(sub)) return 0;
            int r = validate_changed(ns, olds ? olds : Py_None, sub);
            if (r <= 0) return r;
        }
        if (spec_immutable) {
            PyObject* ns = spec ? spec : Py_None;
            PyObject* olds = sget(old, S.spec);
            if (olds == nullptr) olds = Py_None;
            if (ns != olds) {
                int ne = PyObject_RichCompareBool(ns, olds, Py_NE);
                if (ne != 0) return ne < 0 ? -1 : 0;
            }
        }
    }
    // nodeClassRef non-empty CEL rules
    if (spec == nullptr) return 1;
    int spec_true = PyObject_IsTrue(spec);
    if (spec_true < 0) return -1;
    if (!spec_true) return 1;
    if (!PyDict_CheckExact(spec)) return 0;
    PyObject* ref = sget(spec, S.nodeClassRef);
    if (ref == nullptr || !PyDict_Check(ref)) return 1;
    if (!PyDict_CheckExact(ref)) return 0;
    PyObject* fields[3] = {S.group, S.kind, S.name};
    for (PyObject* f : fields) {
        PyObject* v = sget(ref, f);
        if (v == nullptr) continue;
        int eq = PyObject_RichCompareBool(v, S.empty, Py_EQ);
        if (eq != 0) return eq < 0 ? -1 : 0;
    }
    return 1;
}

PyObject* py_crd_valid(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
    if (nargs != 4) {
        PyErr_SetString(PyExc_TypeError,
                        "crd_valid(schema, new, old_or_None, spec_immutable) takes 4 arguments");
        return nullptr;
    }
    int imm = PyObject_IsTrue(args[3]);
    if (imm < 0) return nullptr;
    int r = crd_valid(args[0], args[1], args[2], imm != 0);
    if (r < 0) {
        // whatever went wrong, the Python validator meets it again and
        // reports it its own way
        PyErr_Clear();
        r = 0;
    }
    return PyBool_FromLong(r);
}

PyMethodDef methods[] = {
    {"deep_copy", (PyCFunction)py_deep_copy, METH_O,
     "deep_copy(obj): copy exact dict/list recursively, share everything else."},
    {"json_merge_patch", (PyCFunction)(void (*)(void))py_json_merge_patch, METH_FASTCALL,
     "json_merge_patch(target, patch): RFC 7386 merge patch, returning a new dict."},
    {"merge_patch_owned", (PyCFunction)(void (*)(void))py_merge_patch_owned, METH_FASTCALL,
     "merge_patch_owned(cur, patch): == deep_copy(json_merge_patch(cur, patch)), "
     "sharing the subtrees of cur the patch does not touch."},
    {"crd_valid", (PyCFunction)(void (*)(void))py_crd_valid, METH_FASTCALL,
     "crd_valid(schema, new, old_or_None, spec_immutable): True when CRDValidator "
     "would report no violation."},
    {nullptr, nullptr, 0, nullptr},
};

PyModuleDef moduledef = {
    PyModuleDef_HEAD_INIT, "_jsontree",
    "Native JSON-tree copy, merge patch and CRD validation fast path.", -1, methods,
    nullptr, nullptr, nullptr, nullptr,
};

bool intern_names() {
    struct { PyObject** slot; const char* text; } table[] = {
        {&str_metadata, "metadata"},
        {&S.type, "type"},
        {&S.properties, "properties"},
        {&S.additionalProperties, "additionalProperties"},
        {&S.preserve, "x-kubernetes-preserve-unknown-fields"},
        {&S.required, "required"},
        {&S.items, "items"},
        {&S.maxItems, "maxItems"},
        {&S.enum_set, "_enum_set"},
        {&S.enum_, "enum"},
        {&S.pattern_re, "_pattern_re"},
        {&S.pattern, "pattern"},
        {&S.maxLength, "maxLength"},
        {&S.minLength, "minLength"},
        {&S.minimum, "minimum"},
        {&S.maximum, "maximum"},
        {&S.anyOf, "anyOf"},
        {&S.search, "search"},
        {&S.spec, "spec"},
        {&S.status, "status"},
        {&S.nodeClassRef, "nodeClassRef"},
        {&S.group, "group"},
        {&S.kind, "kind"},
        {&S.name, "name"},
        {&S.empty, ""},
    };
    for (auto& e : table) {
        *e.slot = PyUnicode_InternFromString(e.text);
        if (*e.slot == nullptr) return false;
    }
    return true;
}

}  // namespace

PyMODINIT_FUNC PyInit__jsontree(void) {
    if (!intern_names()) return nullptr;
    return PyModule_Create(&moduledef);
}
