// internal.h — shared host-side structures of libfury_row (not part of the public ABI).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/fury_row.h"

namespace fury {

// How a top-level field is laid out in a row and moved by the device kernels.
enum FieldKind : int32_t {
  kFixed = 0,        // 1/2/4/8-byte scalar in its slot (zero-extended)
  kBool = 1,         // Arrow bit-packed input, putBoolean byte in the slot
  kBytes = 2,        // STRING / BINARY: writeUnaligned into the var section
  kDecimal = 3,      // 16 bytes in the var section (writeDecimal)
  kListFixed = 4,    // LIST of fixed-width (or bool) elements: BinaryArray in the var section
  kOther = 5         // STRUCT / MAP / LIST of var elements: not handled on device yet
};

struct FieldPlan {
  int32_t type_id;
  int32_t width;         // DataTypes.getTypeWidth (-1 for var)
  int32_t kind;          // FieldKind
  int32_t nullable;
  int32_t elem_type;     // LIST element type id
  int32_t elem_width;    // BinaryArrayWriter.elementSize
  int32_t elem_nullable;
};

// Node of the flattened schema tree used by the generic (nested) engine: breadth-first, the
// top-level fields first, every node's children contiguous.
struct GenTpl {
  int32_t type_id;
  int32_t first_child;
  int32_t num_children;
  int32_t nullable;
};

struct OwnedField {
  std::string name;
  int32_t type_id = 0;
  int32_t nullable = 1;
  std::vector<OwnedField> children;
};

}  // namespace fury

struct fury_schema {
  std::vector<fury::OwnedField> fields;
  std::vector<fury::FieldPlan> plan;
  int32_t num_fields = 0;
  int32_t bitmap_bytes = 0;
  int32_t fixed_size = 0;
  int32_t is_fixed = 0;
  int64_t schema_hash = 0;
  int32_t device_ok = 1;          // every field kind has a device kernel
  std::string device_reason;      // why not, when device_ok == 0
  int32_t num_var = 0;            // fields of kind kBytes / kDecimal / kListFixed
  int32_t generic = 0;            // nested schema: encode/decode run the generic engine
  int32_t root = 0;               // 0: rows of the fields; 1 / 2: batches of top-level
                                  // BinaryArrays / BinaryMaps (ArrayEncoder / MapEncoder)
  int32_t depth = 0;              // deepest nesting level (top-level fields = 1)
  std::vector<fury::GenTpl> nodes;
};

// struct fury_decode_plan is defined at the end of kernels.h (it owns device blocks: HIP types).

namespace fury {

// Per-thread last error (fury_last_error).
int set_error(int status, const std::string& msg);
int check_hip(int hip_status, const char* what);

// A path of struct slots resolved against a row schema (schema.cpp; fury_schema_child and
// fury_row_extract share it, rules and messages in include/fury_row.h).
struct ExtractPath {
  const OwnedField* end = nullptr;    // the STRUCT / LIST / MAP field the path reaches
  std::vector<int32_t> nfields;       // per level: fields of the struct whose slot is followed
  int32_t min_size = 0;               // STRUCT: fixed_size of a row of its fields; LIST / MAP: 8
  int32_t exact = 0;                  // STRUCT whose fields are all fixed-width (is_fixed)
};
// `f`: the calling entry point's name, the prefix of every message.
int resolve_extract_path(const fury_schema* s, const int32_t* path, int32_t path_len,
                         const std::string& f, ExtractPath* out);

// The array fury_schema_element / fury_row_explode work on (schema.cpp; rules and messages in
// include/fury_row.h): the LIST / MAP a path reaches in a row schema, or the field of a collection
// schema (path_len 0), and its key / element (side 0) or value (side 1) field.
struct ExplodePath {
  ExtractPath path;                   // row schema: the walk to the LIST / MAP; else empty
  const OwnedField* elem = nullptr;   // the STRUCT / LIST / MAP element field of the chosen array
  int32_t is_map = 0;
  int32_t elem_min = 0;               // STRUCT: fixed_size of a row of its fields; LIST / MAP: 8
  int32_t elem_exact = 0;             // STRUCT whose fields are all fixed-width (is_fixed)
};
int resolve_explode_path(const fury_schema* s, const int32_t* path, int32_t path_len, int32_t side,
                         const std::string& f, ExplodePath* out);

// The map fury_schema_map_side / fury_row_map_split work on (schema.cpp; rules and messages in
// include/fury_row.h): the MAP a path reaches in a row schema, or the field of a MAP collection schema
// (path_len 0).
struct MapPath {
  ExtractPath path;                   // row schema: the walk to the MAP; else empty
  const OwnedField* map = nullptr;
};
int resolve_map_path(const fury_schema* s, const int32_t* path, int32_t path_len,
                     const std::string& f, MapPath* out);
// The slot width of an array's elements: the scalar's width, 8 for a variable-length or nested one.
int32_t element_width(int32_t type_id);

// The selection rules fury_schema_select and fury_row_select share (schema.cpp; rules and messages in
// include/fury_row.h): top-level slots of a row schema, any order, no duplicates, no count limit.
int check_field_selection(const fury_schema* s, const int32_t* fields, int32_t num_selected,
                          const std::string& f);

// The pick rules fury_schema_zip and fury_row_zip share (schema.cpp; rules and messages in
// include/fury_row.h): 1 .. FURY_ZIP_MAX_SOURCES row schemas, picks = (source, top-level slot) pairs,
// any order, no duplicate pair, no count limit.
int check_zip_picks(const fury_schema* const* schemas, int32_t num_sources, const int32_t* picks,
                    int32_t num_picks, const std::string& f);

inline int32_t bitmap_bytes(int64_t n) { return static_cast<int32_t>(((n + 63) / 64) * 8); }
inline int64_t round8(int64_t n) { return (n + 7) & ~int64_t(7); }

}  // namespace fury
